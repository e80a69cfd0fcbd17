/*
 * tfhe_hip.h -- C ABI of the MI355X-native TFHE programmable-bootstrapping engine.
 *
 * Drop-in boundary for the bootstrapping path of Janmajayamall/tfhe-research (Rust crate `tfhe`
 * v0.1.0).  The reference has no FFI of its own (all modules are private, no extern "C"); each
 * entry point below replaces one crate-internal function and takes that function's data in the
 * reference's own memory layout: contiguous row-major u32 ndarrays viewed as `*const u32 + len`
 * (the reference relies on `as_slice().unwrap()`, e.g. bootstrapping.rs:68, key_switching.rs:73).
 * Reference citations are file:line under /root/reference/src.
 *
 * Conventions
 *   - every word is uint32_t, arithmetic wraps mod 2^32 (reference release-mode semantics);
 *   - every call returns an int status (0 = ok); nothing throws or unwinds across this boundary
 *     (the reference signals failure by panicking: assert!/unwrap);
 *   - plain entry points take HOST pointers, block until the result is in host memory, and may
 *     be called from any thread (one context = one stream; do not share a context between
 *     threads without external locking);
 *   - `_device` entry points take DEVICE pointers, enqueue on the context's HIP stream and
 *     return without synchronising; they are graph-capture safe (no allocation, no sync);
 *   - the two unused secret-key arguments of the reference's bootstrap()/and()/or()
 *     (bootstrapping.rs:61-62, boolean.rs:16,39) carry no information and do not cross the ABI.
 */
#ifndef TFHE_HIP_H
#define TFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHE_OK 0
#define TFHE_ERR_INVALID_PARAMS 1   /* parameter set the reference itself could not run */
#define TFHE_ERR_UNSUPPORTED 2      /* valid, but no kernel is instantiated for this shape */
#define TFHE_ERR_NO_KEY 3           /* bootstrapping key not loaded */
#define TFHE_ERR_HIP 4              /* HIP runtime error (see tfhe_last_error) */
#define TFHE_ERR_INVALID_ARGUMENT 5 /* null pointer / bad count / value the reference assert!s on */
#define TFHE_ERR_NO_DEVICE 6        /* no usable GPU: this library has no CPU fallback */
#define TFHE_ERR_EXACTNESS 7        /* parameter set exceeds the exact-NTT bound */
#define TFHE_ERR_IO 8               /* file missing, truncated, not in this format, or corrupt */

/* decomposer.rs:2-6 DecomposerParams */
typedef struct tfhe_decomposer_params {
    uint32_t log_base;
    uint32_t levels;
    uint32_t log_q;
} tfhe_decomposer_params;

/* lib.rs:23-34 TfheParams (noise parameters omitted: they only matter for key generation).
 * glwe_poly_degree is log2(N), exactly as in the reference (lib.rs:40,60). */
typedef struct tfhe_params {
    uint32_t glwe_dimension;   /* k */
    uint32_t glwe_poly_degree; /* log2 N, supported: 9, 10, 11 */
    uint32_t lwe_dimension;    /* n */
    uint32_t padding_bits;
    uint32_t log_p;
    uint32_t log_q;            /* must be 32 */
    tfhe_decomposer_params ks_decomposer;
    tfhe_decomposer_params pbs_decomposer;
} tfhe_params;

typedef struct tfhe_context tfhe_context;

/* Which decomposer of the parameter set an entry point should use. */
#define TFHE_DECOMPOSER_PBS 0
#define TFHE_DECOMPOSER_KS 1

/* ---- parameters / context --------------------------------------------------------------- */

/* lib.rs:101-123 (cfg_test = 0) or lib.rs:77-99 (cfg_test = 1: n = 4) */
void tfhe_params_default(tfhe_params *params, int cfg_test);
/* 0 if the reference could run this parameter set (no underflow / endless loop / shift >= 32) */
int tfhe_params_validate(const tfhe_params *params);

/* Exact-NTT backends.  All give identical bits; they differ in speed and in the parameter sets
 * they can lift exactly (checked at context creation, TFHE_ERR_EXACTNESS otherwise):
 *   FP64_P49   49-bit prime, fp64 arithmetic, the key word taken whole (one spectrum per key
 *              polynomial): half the multiply-accumulate work of FP64; needs
 *              (k+1)*l * N * B * 2^31 < 2^48.25 and (k+1)*l <= 20 -- small gadget bases, e.g. the
 *              reference's default parameters (N = 512, k = 2, l = 6, log_base = 4)
 *   FP64       42-bit prime, fp64 arithmetic, key split into 16-bit halves; needs
 *              (k+1)*l * N * B * 2^15 < 2^40.9 and log_base <= 9
 *   GOLDILOCKS p = 2^64 - 2^32 + 1, u64 arithmetic; needs (k+1)*l * N * B * 2^32 < 2^62
 *   GOLDILOCKS_SPLIT  the same field with the key split into 16-bit halves; needs
 *              (k+1)*l * N * B * 2^15 < 2^62, which every base the reference can express satisfies
 *   AUTO       the first of FP64_FFT (below), FP64_P49, FP64, GOLDILOCKS, GOLDILOCKS_SPLIT whose bound holds
 *              (env TFHE_HIP_BACKEND=fp64-fft|fp64-p49|fp64|goldilocks|goldilocks-split overrides AUTO). */
#define TFHE_BACKEND_AUTO 0
#define TFHE_BACKEND_GOLDILOCKS 1
#define TFHE_BACKEND_FP64 2
#define TFHE_BACKEND_GOLDILOCKS_SPLIT 3
#define TFHE_BACKEND_FP64_P49 4
/* FP64_FFT: the negacyclic product through a complex FFT in fp64 (N/2 points, two coefficients per element,
 *            key split into 16-bit halves), exact by a proven bound on the rounding error of every output
 *            coefficient (csrc/field_fft.h: (3 n eta + sqrt 2 (R + 1) u) R M^1.5 |x| |y| < 1/4, e.g. 0.013 at N = 1024,
 *            k = 1, l = 3, log_base = 7).  Same bits as the exact-NTT fields. */
#define TFHE_BACKEND_FP64_FFT 5

/* Creates a context bound to HIP device `device`.  Fails with TFHE_ERR_NO_DEVICE when no GPU is
 * present: there is deliberately no CPU path behind this ABI. */
int tfhe_context_create(const tfhe_params *params, int device, tfhe_context **out);
int tfhe_context_create_with_backend(const tfhe_params *params, int device, int backend,
                                     tfhe_context **out);
/* "fp64-fft", "fp64-p49", "fp64-p42", "goldilocks" or "goldilocks-split" */
const char *tfhe_context_backend(const tfhe_context *ctx);
void tfhe_context_destroy(tfhe_context *ctx);
/* Run on an existing hipStream_t, e.g. torch.cuda.current_stream().cuda_stream.  A NULL handle is
 * HIP's default stream (that is what torch hands out unless the caller switched streams).  A new
 * context starts on a private non-blocking stream; tfhe_context_use_own_stream goes back to one.
 * Whatever the stream, everything a call enqueues is ordered on it: the blind rotation of a large batch
 * forks half of its launches onto a second, context-owned stream and joins it again before the call
 * returns (events; tfhe_debug_blind_rotate_plan).  During a stream capture it stays on the one stream. */
int tfhe_context_set_stream(tfhe_context *ctx, void *hip_stream);
int tfhe_context_use_own_stream(tfhe_context *ctx);
int tfhe_context_synchronize(tfhe_context *ctx);
/* Pre-sizes the per-batch workspace so that later _device calls up to `max_batch` never allocate.
 * A call beyond the reservation (a host form of a larger batch, a larger tfhe_context_reserve) frees the
 * workspace and allocates a larger one.  A captured graph (hipGraph) of _device calls has the workspace's
 * device pointers baked in, so reserve the largest batch BEFORE capturing: a graph captured earlier must
 * not be replayed after the workspace grew (it would touch freed memory), it has to be captured again. */
int tfhe_context_reserve(tfhe_context *ctx, size_t max_batch);
const char *tfhe_last_error(const tfhe_context *ctx);
const char *tfhe_status_string(int status);

/* ---- key upload: BootstrappingKey (bootstrapping.rs:18-21) ------------------------------- */
/* bsk: the n GGSW ciphertexts of lwe_sk_ggsw_enc back to back, [n][(k+1)*l][k+1][N]
 *      (ggsw.rs:37-41: row = poly_index*l + level, each row one GLWE, body last);
 * ksk: KeySwitchingKey.data, [k*N*l_ks][n+1] (key_switching.rs:13-15).
 * The device keeps the BSK in the NTT domain (u64, pre-scaled by 1/N) and the KSK as is. */
int tfhe_load_bootstrapping_key(tfhe_context *ctx, const uint32_t *bsk, const uint32_t *ksk);
int tfhe_load_bootstrapping_key_device(tfhe_context *ctx, const uint32_t *bsk, const uint32_t *ksk);

/* Unrolled blind rotation (the crate only sketches it: notes/BMMP Bootstrapping.md:13-25).  Two key
 * bits are consumed per step with three GGSWs per pair,
 *   bsk_bmmp [n/2][3][(k+1)*l][k+1][N]:  GGSW(s_2j s_2j+1), GGSW(s_2j (1 - s_2j+1)), GGSW(s_2j+1 (1 - s_2j)),
 *   acc += sum_{m<3} (X^{e_m} - 1) * external_product(bsk_bmmp[j][m], acc),  e = (a_2j + a_2j+1, a_2j, a_2j+1):
 * half the decompositions and forward transforms for a 1.5x key.  Loading such a key puts the
 * context into this mode (tfhe_bootstrap_batch, tfhe_blind_rotate_batch, the gates ... then run it);
 * loading an ordinary key switches back.  NOT the reference's bootstrap(): same plaintext, different
 * key material, different ciphertext bits (checked against oracle.bootstrap_bmmp instead).  Needs
 * even n, N = 512 and a context in the GOLDILOCKS or FP64_P49 backend -- the fields where its three accumulator
 * sets fit the registers: +10 % / -5 % against the loop there, 1.9-3.4x slower on 50-172 spilled registers in the
 * two-spectra fields, where it is refused (TFHE_ERR_UNSUPPORTED otherwise, with the reason in tfhe_last_error). */
int tfhe_load_bootstrapping_key_bmmp(tfhe_context *ctx, const uint32_t *bsk_bmmp, const uint32_t *ksk);
int tfhe_load_bootstrapping_key_bmmp_device(tfhe_context *ctx, const uint32_t *bsk_bmmp, const uint32_t *ksk);
/* 1 if the loaded key is a BMMP key */
int tfhe_context_uses_bmmp(const tfhe_context *ctx);

/* ---- bootstrap(): bootstrapping.rs:58-120 ------------------------------------------------- */
/* lwe_in  [batch][n+1]   LweCiphertext.data (a_0..a_{n-1}, b)              (lwe.rs:110-115)
 * test_vector_poly [tv_count][N], tv_count = 1 (shared) or batch; un-encoded values < 2^log_p,
 *         as produced by construct_test_from_lut (encoded on the device: glwe.rs:141-151)
 * lwe_out [batch][n+1] */
int tfhe_bootstrap_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch,
                         const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);
int tfhe_bootstrap_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch,
                                const uint32_t *test_vector_poly, size_t tv_count,
                                uint32_t *lwe_out);

/* Blind rotation only (bootstrapping.rs:67-105): glwe_out [batch][k+1][N] */
int tfhe_blind_rotate_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch,
                            const uint32_t *test_vector_poly, size_t tv_count, uint32_t *glwe_out);
int tfhe_blind_rotate_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch,
                                   const uint32_t *test_vector_poly, size_t tv_count,
                                   uint32_t *glwe_out);

/* ---- blind rotation and bootstrap from a GLWE accumulator (no reference counterpart) -------------------------------
 * The reference's rotation starts from a clear test vector (bootstrapping.rs:67-78).  Here the initial accumulator is
 * any GLWE ciphertext: acc_in [acc_count][k+1][N], acc_count = 1 (every row starts from the same one) or batch.  All
 * arithmetic mod 2^32:
 *   acc_0 = X^{(2N - b~ - rotation_offset) mod 2N} * acc_in,  b~ = switch_modulus(b, 32, log2(2N)), rotation_offset < 2N
 *     -- the negacyclic monomial product on all k+1 polynomials; the words of acc_in are taken as they are (already
 *     encoded: no shift by 32 - log_p - padding_bits);
 *   then the n CMUXes of bootstrapping.rs:79-105, unchanged.
 * tfhe_blind_rotate_glwe_batch* returns the final accumulators, lwe_in [batch][n+1] -> glwe_out [batch][k+1][N].
 * tfhe_bootstrap_glwe_batch* adds sample extraction at index 0 and the key switch like tfhe_bootstrap_batch*, in the
 * order tfhe_context_set_bootstrap_order selected (KS first: input and output have k*N+1 words).  The result's phase
 * is coefficient (phase(lwe_in) 2N / 2^32 + rotation_offset) mod 2N of phase(acc_in), negated from N on.
 *
 * With acc_in = (0, .., 0, tv << (32 - log_p - padding_bits)), acc_count = tv_count and rotation_offset 0 the words
 * equal tfhe_blind_rotate_batch's and tfhe_bootstrap_batch's bit for bit.  What it adds: the table may stay secret
 * (a GLWE encryption of the encoded test vector), and a packed GLWE of results (tfhe_pack_lwe_batch) is bootstrapped
 * again without unpacking: with 2^log_p results on N / 2^log_p coefficients each, rotation_offset = N / 2^(log_p+1)
 * selects the one the input encrypts (the tree LUT below).  No new exactness rule: from the first CMUX on the products'
 * inputs are arbitrary words already.  Noise: the rotation's own plus that of the selected coefficient of acc_in.
 *
 * Every kernel shape and backend the context was admitted with; the kernels are the ones of tfhe_blind_rotate_batch
 * (their accumulator set-up reads acc_in through the rotated index).  With a BMMP key loaded: TFHE_ERR_UNSUPPORTED.
 * acc_in may not overlap glwe_out.  The _device forms run on the context's stream, allocate nothing after
 * tfhe_context_reserve(max_batch) and are capturable wherever tfhe_bootstrap_batch_device is. */
int tfhe_blind_rotate_glwe_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, const uint32_t *acc_in,
                                 size_t acc_count, size_t rotation_offset, uint32_t *glwe_out);
int tfhe_blind_rotate_glwe_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, const uint32_t *acc_in,
                                        size_t acc_count, size_t rotation_offset, uint32_t *glwe_out);
int tfhe_bootstrap_glwe_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, const uint32_t *acc_in,
                              size_t acc_count, size_t rotation_offset, uint32_t *lwe_out);
int tfhe_bootstrap_glwe_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, const uint32_t *acc_in,
                                     size_t acc_count, size_t rotation_offset, uint32_t *lwe_out);

/* sample_extract(): bootstrapping.rs:122-156.  glwe [batch][k+1][N] -> lwe_out [batch][k*N+1] */
int tfhe_sample_extract_batch(tfhe_context *ctx, const uint32_t *glwe, size_t batch,
                              size_t sample_index, uint32_t *lwe_out);

/* key_switch_lwe(): key_switching.rs:63-103 with the loaded KSK (from dimension k*N to n).
 * lwe_in [batch][k*N+1] -> lwe_out [batch][n+1] */
int tfhe_key_switch_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch,
                          uint32_t *lwe_out);
int tfhe_key_switch_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch,
                                 uint32_t *lwe_out);

/* ---- packing key switch (no reference counterpart): many LWE results into one GLWE ciphertext ---
 * Pack(c_0 .. c_{m-1}) = (0, .., 0, sum_j b_j X^j) - sum_{i<d} sum_{l<l_ks} dec_l(A_i) (*) PK[i*l_ks + l] with
 * A_i(X) = sum_j a_j,i X^j, dec_l the KS decomposer's signed digit of level l coefficient by coefficient and (*) the
 * negacyclic product with every component of the key row.  Coefficient j of the result decrypts (under the GLWE key)
 * to what c_j decrypts to, coefficients >= m to 0; sample_extract(.., j) + key switch gives an LWE of message j again.
 * m LWEs of d+1 words become (k+1) N words: the inverse direction of tfhe_sample_extract_batch.
 *
 * Packing key: pksk [from_dimension*l_ks][k+1][N], row i*l_ks + l a GLWE encryption under glwe_sk of the constant
 * polynomial from_sk[i] * g_l (g_l: the gadget factor tfhe_generate_ksk uses, in the context's alignment mode).
 * tfhe_generate_packing_key completes a buffer pre-filled row by row like tfhe_glwe_encrypt_zero_batch (masks uniform,
 * body = error); from_sk [from_dimension] and glwe_sk [k][N] are binary host arrays; the _device form takes pksk on the
 * device.  tfhe_load_packing_key prepares the key and keeps it in the context, independently of the bootstrapping
 * key; it also sizes the workspace, so that tfhe_pack_lwe_batch_device never allocates or synchronises (everything is
 * ordered on the context's stream; safe under stream capture).
 *
 * Exactness: a call sums (k+1) l_ks key rows at a time in the backend's transform domain -- the external product's
 * shape with the KS decomposer.  Where the backend's bound does not hold for that shape, tfhe_load_packing_key*
 * returns TFHE_ERR_EXACTNESS with the reason in tfhe_last_error; nothing is computed outside a proven bound.
 *
 * Noise: every output coefficient carries the noise of its input plus, per coefficient, variance
 *   d * l_ks * m * E[digit^2] * (sigma_glwe * 2^32)^2      (the key rows' errors, E[digit^2] ~ B^2/12)
 *   + (d/2) * 2^(2*ignored_bits_ks) / 12                  (rounding to the decomposer's precision, binary key)
 * in units of the 32-bit torus; m = per_group.
 *
 * lwe_in [groups][per_group][from_dimension+1], 1 <= per_group <= N; glwe_out [groups][k+1][N].
 * TFHE_ERR_NO_KEY before a packing key is loaded. */
int tfhe_generate_packing_key(tfhe_context *ctx, const uint32_t *from_sk, size_t from_dimension,
                              const uint32_t *glwe_sk, uint32_t *pksk);
int tfhe_generate_packing_key_device(tfhe_context *ctx, const uint32_t *from_sk, size_t from_dimension,
                                     const uint32_t *glwe_sk, uint32_t *pksk);
int tfhe_load_packing_key(tfhe_context *ctx, const uint32_t *pksk, size_t from_dimension);
int tfhe_load_packing_key_device(tfhe_context *ctx, const uint32_t *pksk, size_t from_dimension);
/* dimension of the LWE key the loaded packing key packs from: tfhe_pack_lwe_batch* reads from_dimension+1 words per
 * ciphertext, so a caller that holds shaped arrays checks their width against it; TFHE_ERR_NO_KEY if none is loaded */
int tfhe_packing_key_dimension(const tfhe_context *ctx, size_t *from_dimension);
int tfhe_pack_lwe_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t groups, size_t per_group,
                        uint32_t *glwe_out);
int tfhe_pack_lwe_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t groups, size_t per_group,
                               uint32_t *glwe_out);

/* ---- GLWE key switching and automorphisms (no reference counterpart): X -> X^t in one fused launch ------------------
 * Ring Z_{2^32}[X] / (X^N + 1).  For odd t in [1, 2N), sigma_t(p)(X) = p(X^t): coefficient j of p lands on index
 * j*t mod N, negated when j*t mod 2N >= N.  Gather form, with u = t^-1 mod 2N: sigma_t(p)[m] = p[m*u mod 2N] if that
 * index is < N, else -p[(m*u mod 2N) - N].  The sigma_t are exactly the signed coefficient permutations that respect the
 * ring's product: t = 2N-1 reverses, and x + sigma_t(x) is one step of the trace (below).
 *
 * A switch key for polynomials F_0 .. F_{k-1} with coefficients in {-1, 0, 1} is key [k*l_ks][k+1][N]: row i*l_ks + l
 * a GLWE encryption under the context's GLWE key S of F_i(X) * g_l, g_l the KS decomposer's gadget factor in the
 * context's alignment mode exactly as tfhe_generate_packing_key uses it (a coefficient -1 adds 0 - g_l).
 * F = sigma_t(S) (tfhe_glwe_sk_automorphism) gives the automorphism key for t; F = S' (binary) the key that switches
 * from S' to S.  For c = (A_0 .. A_{k-1}, B):
 *
 *   Auto_t(c; KEY) = (0, .., 0, sigma_t(B)) - sum_{i<k} sum_{l<l_ks} dec_l(sigma_t(A_i)) (*) KEY[i*l_ks + l]
 *
 * with dec_l and (*) as in the packing formula above.  With add_input the input ciphertext is added to the result in
 * wrapping 32-bit words: x + Auto_t(x), one trace step.  t = 1 is the plain GLWE key switch.  An automorphism turns
 * a ciphertext under S into one under sigma_t(S) and is usable only together with the switch back: key == NULL is the
 * bare permutation (one elementwise launch, the result under sigma_t(S); add_input is refused), for clients and tests.
 *
 * Identity.  Under a noise-free key, for any masks, phi_S(Auto_t(c)) = sigma_t(B) - sum_i F_i (*) Rec(sigma_t(A_i)),
 * Rec the decomposer's recomposition coefficient by coefficient.  Where no bits are ignored this is sigma_t(phi_S(c))
 * exactly (F = sigma_t(S)); with the aligned decomposer and ig ignored bits it holds within k*N*2^(ig-1); the literal
 * decomposer at bases that do not divide 32 keeps its known quirk and only the Rec form holds.
 *
 * Partial trace.  Step j = 1..s applies x <- x + Auto_{t_j}(x) with t_j = N/2^(j-1) + 1.  After s steps a coefficient
 * whose index is a multiple of 2^s holds 2^s TIMES its value and every other coefficient holds 0 -- cleared without
 * knowing any of them, which no product with a clear mask can do.  The factor 2^s is unavoidable (N has no inverse mod
 * 2^32): it comes out of the caller's scale, so encode s bits below the scale the result is read at.
 *
 * Noise.  An output coefficient carries its permuted input's noise (on a kept coefficient of a trace step exactly
 * twice the input's: the same error is added to itself) plus variance
 *   s_ks^2 = k * l_ks * N * (B_ks^2/12 + 1/6) * (sigma_glwe * 2^32)^2 + (k*N/2) * 2^(2*ignored_bits_ks) / 12
 * in units of the 32-bit torus: the packing formula's with d*m replaced by k polynomials of N coefficients.  After s
 * trace steps: 4^s * var_in + s_ks^2 * (4^s - 1) / 3.
 *
 * Exactness: the product sums ONE slice of (k+1) l_ks rows in the KS base -- the packing key's rule, unchanged.  A
 * backend that refuses a packing key under the context's parameters refuses a switch key
 * (tfhe_prepare_glwe_switch_key*: TFHE_ERR_EXACTNESS, the reason in tfhe_last_error); nothing is computed outside a
 * proven bound.
 *
 * tfhe_generate_glwe_switch_key completes a buffer pre-filled row by row like tfhe_glwe_encrypt_zero_batch (masks
 * uniform, body = error); from_polys [k][N] (int32, entries in {-1, 0, 1}, else TFHE_ERR_INVALID_ARGUMENT) and glwe_sk
 * [k][N] (binary) are host arrays; the _device form takes key on the device.  tfhe_glwe_sk_automorphism is host-only
 * arithmetic: out [k][N] = sigma_t(glwe_sk).  tfhe_prepare_glwe_switch_key makes an opaque handle that owns the
 * prepared key on the device (this one call synchronises).  The handle belongs to the context that made it -- another
 * context's or backend's is TFHE_ERR_INVALID_ARGUMENT --, is independent of the bootstrapping and the packing key
 * (loading either leaves it valid), and is destroyed by the caller (NULL is allowed) before its context.  Any number
 * may live at once; a trace needs log2 N at most.
 *
 * glwe_in, glwe_out [batch][k+1][N], 1 <= batch < 2^31; glwe_out may BE glwe_in (any other overlap is refused).  One
 * launch of `batch` teams: no workspace, nothing allocated or synchronised, so the _device form can be captured as it
 * stands.  An even t or t >= 2N is TFHE_ERR_INVALID_ARGUMENT with the reason in tfhe_last_error. */
typedef struct tfhe_glwe_switch_key tfhe_glwe_switch_key;
int tfhe_glwe_sk_automorphism(const uint32_t *glwe_sk, size_t k, unsigned log_n, size_t t, int32_t *out);
int tfhe_generate_glwe_switch_key(tfhe_context *ctx, const int32_t *from_polys, const uint32_t *glwe_sk, uint32_t *key);
int tfhe_generate_glwe_switch_key_device(tfhe_context *ctx, const int32_t *from_polys, const uint32_t *glwe_sk,
                                         uint32_t *key);
int tfhe_prepare_glwe_switch_key(tfhe_context *ctx, const uint32_t *key, tfhe_glwe_switch_key **out);
int tfhe_prepare_glwe_switch_key_device(tfhe_context *ctx, const uint32_t *key, tfhe_glwe_switch_key **out);
void tfhe_glwe_switch_key_destroy(tfhe_glwe_switch_key *key);
int tfhe_glwe_automorphism_batch(tfhe_context *ctx, const uint32_t *glwe_in, size_t batch, size_t t,
                                 const tfhe_glwe_switch_key *key, int add_input, uint32_t *glwe_out);
int tfhe_glwe_automorphism_batch_device(tfhe_context *ctx, const uint32_t *glwe_in, size_t batch, size_t t,
                                        const tfhe_glwe_switch_key *key, int add_input, uint32_t *glwe_out);

/* ---- multi-bit blind rotation (no reference counterpart): g key bits per external product, for small batches -------
 * The multi-bit blind rotation of Joye and Paillier (2022).  A blind rotation's latency is the number of SEQUENTIAL
 * external products times the latency of one; this variant runs ceil(n / g) of them instead of n, and what it adds --
 * forming one GGSW per (sample, group of g key bits), the BUNDLE -- is independent work for the CUs a small batch leaves
 * idle.  Opt-in: a separate key handle and separate entry points; the context's loaded key and every other entry point
 * are untouched.  All arithmetic is mod 2^32.
 *
 * Groups and patterns.  g in {2, 3, 4}; G = ceil(n / g) groups; group i covers key bits g*i .. min(n, g*i + g) - 1, g_i of
 * them (the last group may be ragged).  A pattern is an integer p in [1, 2^g_i): bit j of p stands for key bit g*i + j.
 *
 * Key.  bsk_mb [G][2^g - 1][(k+1)*l][k+1][N]: slot (i, p - 1) is a GGSW in the reference's layout (ggsw.rs:37-41) that
 * encrypts  prod_{j in p} s_{g*i+j} * prod_{j not in p, j < g_i} (1 - s_{g*i+j})  in {0, 1}: "the group's bits are exactly
 * p".  Slots of a ragged group with p >= 2^g_i are never read (tfhe_generate_multibit_key encrypts 0 there).  The pattern
 * "no bit set" needs no GGSW: the indicators of a group sum to 1, which is why the step below is acc + ...
 *
 * Rotation.  a~_m = switch_modulus_2n(a_m) and b~ are the bootstrap's own; e_{i,p} = sum_{j in p} a~_{g*i+j} mod 2N.
 * acc_0 is the bootstrap's, X^(-b~) * (0, .., 0, tv << tv_shift), or the rotated GLWE accumulator of
 * tfhe_blind_rotate_glwe_batch (acc_in, rotation_offset).  For i = 0 .. G - 1:
 *   Bundle_i[r][c][.] = sum_p ( X^(e_{i,p}) * K_{i,p}[r][c] - K_{i,p}[r][c] )    wordwise wrapping u32, the negacyclic shift
 *                       of utils.rs:183-207, over all (k+1)*l rows and k+1 columns
 *   acc <- acc + external_product(Bundle_i, acc)                                  ggsw.rs:132-161 with the PBS decomposer,
 *                                                                                 literal or aligned as the context is set
 * Output: the GLWE accumulator and / or sample_extract(., 0).  The bundle is formed on the RAW key words before it is
 * transformed, so it is an ordinary GGSW of arbitrary words: the context's exactness rule covers it as it covers any
 * bootstrapping key, and the result is byte for byte "bundle, tfhe_external_product_batch, wrapping add" repeated G times.
 * The bootstrap form adds the context's key switch after the rotation or before it, as tfhe_context_set_bootstrap_order
 * says: byte for byte tfhe_key_switch_batch_device composed with the rotation.
 *
 * This is NOT the reference's bootstrap(): the plaintext is the same, the key material and the ciphertext bits differ
 * (as with a BMMP key).
 *
 * Identity.  Under noise-free GGSWs and with no ignored bits, phi_S(acc_final) = X^(rho - b~) * phi_S(acc_0) exactly,
 * rho = sum_m a~_m s_m.  With the aligned decomposer and ig ignored bits a step rounds every word of acc by at most
 * 2^(ig-1), the phase of the rounded accumulator moves by at most (1 + k*N) 2^(ig-1), and the step's message X^rho_i - 1
 * is two monomials: within G * 2 * (1 + k*N) * 2^(ig-1) per coefficient after the G steps.
 *
 * Noise (derived, then compared with measurements: DESIGN.md).  A bundle row's error is sum_p (X^e - 1) e_p, variance
 * 2 (2^g_i - 1) sigma^2, and its message X^(sum a~ s) - 1 is two monomials, so the decomposer's rounding counts twice.
 * Per group, in units of the 32-bit torus:
 *   2 (2^g_i - 1) (k+1) l N (B^2/12 + 1/6) (sigma_glwe 2^32)^2  +  2 (1 + k N / 2) 2^(2 ig_pbs) / 12
 * and s_mb^2 is the sum over the groups; the modulus-switch and key-switch terms are the bootstrap's.  Against the
 * ordinary rotation's s_br^2 that is about 2 (2^g - 1) / g: 3x, 4.7x, 7.5x the variance for g = 2, 3, 4 -- the price of
 * the shorter chain and the reason it is opt-in.
 *
 * Offered where the launcher offers the wide team: the fp64-fft backend, N <= 1024, (k+1) l row buffers within a CU's LDS;
 * elsewhere tfhe_prepare_multibit_key* and tfhe_context_reserve_multibit return TFHE_ERR_UNSUPPORTED with the reason in
 * tfhe_last_error.  g outside {2, 3, 4}, a NULL pointer, an empty batch, one beyond 65535 or beyond the reservation:
 * TFHE_ERR_INVALID_ARGUMENT.
 *
 * tfhe_generate_multibit_key completes a buffer pre-filled like tfhe_ggsw_encrypt_batch's (every GLWE row: masks uniform,
 * body = error); its words equal tfhe_ggsw_encrypt_batch with the indicator products as messages.  lwe_sk [n] and glwe_sk
 * [k][N] are host arrays and must be binary; the _device form takes bsk_mb on the device.  tfhe_prepare_multibit_key makes
 * an opaque handle that owns the raw key on the device (this one call synchronises).  The handle belongs to the context
 * that made it -- another context's is TFHE_ERR_INVALID_ARGUMENT --, is independent of the loaded bootstrapping key, and is
 * destroyed by the caller (NULL is allowed) before its context.  Any number may live at once, with different g.
 *
 * tfhe_context_reserve_multibit reserves the bundle workspace, max_batch * G * prepared-GGSW bytes (41 MB per sample at
 * k = 1, N = 1024, n = 630, l = 3, g = 3), and the LWE workspace of tfhe_context_reserve.  The host forms reserve what they
 * need; a _device call beyond the reservation is refused and names its need in bytes.  After it the _device forms allocate
 * nothing, stay on the context's stream and can be captured: two launches per rotation (bundles: one workgroup per four
 * bundle polynomials and sample; rotation: one wide team per sample), plus the key switch in the bootstrap form.
 *
 * lwe_in [batch][n+1] (the bootstrap form: the context's boundary dimension).  Pass EITHER test_vector_poly [tv_count][N]
 * (clear, tv_count 1 or batch) OR acc_in [tv_count][k+1][N] with rotation_offset < 2N; the other is NULL.  Pass glwe_out
 * [batch][k+1][N], lwe_extracted [batch][k*N+1] or both.  The bootstrap form is TFHE_ERR_NO_KEY while the context holds
 * no key-switching key.  With tfhe_context_set_timing, tfhe_multibit_last_kernel_ms reports the two launches of the last
 * tfhe_multibit_blind_rotate_batch[_device] separately. */
typedef struct tfhe_multibit_key tfhe_multibit_key;
int tfhe_generate_multibit_key(tfhe_context *ctx, const uint32_t *lwe_sk, const uint32_t *glwe_sk, unsigned g, uint32_t *bsk_mb);
int tfhe_generate_multibit_key_device(tfhe_context *ctx, const uint32_t *lwe_sk, const uint32_t *glwe_sk, unsigned g,
                                      uint32_t *bsk_mb);
int tfhe_prepare_multibit_key(tfhe_context *ctx, const uint32_t *bsk_mb, unsigned g, tfhe_multibit_key **out);
int tfhe_prepare_multibit_key_device(tfhe_context *ctx, const uint32_t *bsk_mb, unsigned g, tfhe_multibit_key **out);
void tfhe_multibit_key_destroy(tfhe_multibit_key *key);
int tfhe_context_reserve_multibit(tfhe_context *ctx, size_t max_batch, unsigned g);
int tfhe_multibit_blind_rotate_batch(tfhe_context *ctx, const tfhe_multibit_key *key, const uint32_t *lwe_in, size_t batch,
                                     const uint32_t *test_vector_poly, size_t tv_count, const uint32_t *acc_in,
                                     size_t rotation_offset, uint32_t *glwe_out, uint32_t *lwe_extracted);
int tfhe_multibit_blind_rotate_batch_device(tfhe_context *ctx, const tfhe_multibit_key *key, const uint32_t *lwe_in, size_t batch,
                                            const uint32_t *test_vector_poly, size_t tv_count, const uint32_t *acc_in,
                                            size_t rotation_offset, uint32_t *glwe_out, uint32_t *lwe_extracted);
int tfhe_multibit_bootstrap_batch(tfhe_context *ctx, const tfhe_multibit_key *key, const uint32_t *lwe_in, size_t batch,
                                  const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);
int tfhe_multibit_bootstrap_batch_device(tfhe_context *ctx, const tfhe_multibit_key *key, const uint32_t *lwe_in, size_t batch,
                                         const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);
int tfhe_multibit_last_kernel_ms(tfhe_context *ctx, float *bundle_ms, float *rotate_ms);

/* ---- block-binary blind rotation (no reference counterpart): b key bits per decomposition, for large batches ----------
 * The blind rotation of Lee, Min, Seo and Song, "Faster TFHE Bootstrapping with Block Binary Keys" (2023).  The LWE secret
 * is drawn with AT MOST ONE 1 per block of b consecutive bits.  Over the bits j of one block that makes
 *   X^(sum_j a~_j s_j) = 1 + sum_j s_j (X^(a~_j) - 1),
 * so the b external products of a block are all taken of the SAME accumulator: they share one rounding, one digit chain
 * and one set of forward transforms, and -- the monomial factors being pointwise in the transform domain -- one
 * accumulator set, one pair of inverse transforms and one lift.  The key is the context's loaded, ORDINARY bootstrapping
 * key (n GGSWs of the bits, the reference's layout, tfhe_generate_keys / tfhe_load_bootstrapping_key): only the secret's
 * distribution and the rotation's formula change.  No key type, no per-sample workspace.  All arithmetic is mod 2^32.
 * Whether a block-binary secret of dimension n reaches a given security level is not this library's claim: the paper
 * treats it, and choosing n is the caller's business.
 *
 * Definition.  block = b >= 2.  Block i covers key bits b*i .. min(n, b*i + b) - 1 (the last block may be ragged).
 * a~_m = switch_modulus_2n(a_m) and b~ are the bootstrap's own; acc_0 is the bootstrap's, X^(-b~) * (0, .., 0, tv << tv_shift),
 * or the rotated GLWE accumulator of tfhe_blind_rotate_glwe_batch (acc_in, rotation_offset), as
 * tfhe_multibit_blind_rotate_batch takes them.  For every block in turn:
 *   P_j  = external_product(BSK_j, acc)           ggsw.rs:132-161 with the PBS decomposer, literal or aligned as the context
 *                                                 is set; every P_j of a block from the SAME acc
 *   acc <- acc + sum_j ( X^(a~_j) * P_j - P_j )    the negacyclic shift of utils.rs:183-207, wrapping u32
 * Output: the GLWE accumulator and / or sample_extract(., 0).  The words are, byte for byte, tfhe_external_product_batch,
 * tfhe_glwe_mul_monomial_batch and wrapping adds composed that way.  The bootstrap form adds the context's key switch after
 * the rotation or before it, as tfhe_context_set_bootstrap_order says.
 *
 * This is NOT the reference's bootstrap(): the plaintext is the same (for a block-binary secret), the ciphertext bits
 * differ.  With b = 1 it would still not be the ordinary CMUX, which decomposes the rotated difference X^a~ acc - acc, not
 * acc; b = 1 is refused.
 *
 * Identity.  Under noise-free GGSWs and a block-binary secret, phi_S(acc_final) = X^(rho - b~) * phi_S(acc_0),
 * rho = sum_m a~_m s_m, within ceil(n/b) * 2 * (1 + k*N) * 2^(ig-1) per coefficient (ig ignored bits; exactly with none): a
 * step rounds every word of acc once, by at most 2^(ig-1), and the step's message X^rho_i - 1 is two monomials.  A secret
 * with two 1s in one block does NOT satisfy it.
 *
 * Noise.  Per key bit the external product's variance counts twice, for (X^a~ - 1); per block the decomposer's rounding
 * counts twice.  In units of the 32-bit torus:
 *   s_bb^2 = 2 n (k+1) l N (B^2/12 + 1/6) (sigma_glwe 2^32)^2  +  2 ceil(n/b) (1 + k N / 2) 2^(2 ig_pbs) / 12
 * about twice the ordinary rotation's variance (against 3x - 7.5x for the multi-bit rotation).  The modulus-switch and
 * key-switch terms are the bootstrap's.
 *
 * Exactness.  The b (k+1) l products of a block are summed in the transform domain, each with a factor of modulus <= 2:
 * FftField::block_error_bound (csrc/field_fft.h) below 1/4 admits b.  tfhe_block_rotate_max_block returns the largest
 * admitted b (6 at k = 1, N = 1024, B = 2^7, l = 3), or 0 with the reason in tfhe_last_error and the status that says why;
 * a block above it is TFHE_ERR_EXACTNESS and names the largest admitted one.
 *
 * Offered in the fp64-fft backend with one wave per polynomial, N = 512 and N = 1024, on an ordinary key:
 * TFHE_ERR_UNSUPPORTED with the reason for the prime-field backends, N = 2048 and a BMMP-loaded key.  block < 2, a NULL
 * pointer, an empty batch, both or neither of test_vector_poly / acc_in: TFHE_ERR_INVALID_ARGUMENT.  No loaded key:
 * TFHE_ERR_NO_KEY.
 *
 * One team of k+1 waves rotates one sample at EVERY batch size: the batches the ordinary rotation gives to the wide team
 * or to the pair kernel run on this team kernel too.  Large batches go out as the ordinary rotation's do -- chunks,
 * segments over slices of the key with the accumulators parked in the workspace of tfhe_context_reserve, two streams --
 * with every segment a whole number of blocks.  After tfhe_context_reserve the _device forms allocate nothing, stay on the
 * context's stream and can be captured.
 *
 * lwe_in [batch][n+1] (the bootstrap form: the context's boundary dimension).  Pass EITHER test_vector_poly [tv_count][N]
 * (clear, tv_count 1 or batch) OR acc_in [tv_count][k+1][N] with rotation_offset < 2N; the other is NULL.  Pass glwe_out
 * [batch][k+1][N], lwe_extracted [batch][k*N+1] or both. */
int tfhe_block_rotate_max_block(tfhe_context *ctx, unsigned *max_block);
int tfhe_block_blind_rotate_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned block,
                                  const uint32_t *test_vector_poly, size_t tv_count, const uint32_t *acc_in,
                                  size_t rotation_offset, uint32_t *glwe_out, uint32_t *lwe_extracted);
int tfhe_block_blind_rotate_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned block,
                                         const uint32_t *test_vector_poly, size_t tv_count, const uint32_t *acc_in,
                                         size_t rotation_offset, uint32_t *glwe_out, uint32_t *lwe_extracted);
int tfhe_block_bootstrap_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned block,
                               const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);
int tfhe_block_bootstrap_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned block,
                                      const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);

/* ---- tree LUT: a function of d digits of log_p bits each (no reference counterpart) ---------------------------------
 * The tree-based bootstrap of Guimaraes, Borin and Aranha (2021).  Inputs and output are ordinary LWE ciphertexts at
 * the bootstrap boundary, so it composes with gates, gate graphs and itself; its noise does not depend on the table
 * size.  B = 2^log_p, rep = N / B; digits[t] [batch][io_words] encrypts digit x_t < B (digit 0 least significant),
 * table [table_sets][tables][B^d] holds un-encoded values < B, table_sets = 1 or batch; every intermediate LWE is a
 * k N-dimensional sample extraction:
 *   R0_h = sample_extract(BlindRotate(c_0; construct_test_from_lut(T[h B .. h B + B))), 0)        for h < B^(d-1)
 *   for t = 1 .. d-1 and h < B^(d-1-t):
 *     G_h  = Pack(L_0 .. L_{N-1}),  L_j = R(t-1)_{h B + floor(j / rep)}   (the packing formula above with per_group = N:
 *            result v occupies coefficients [v rep, (v+1) rep))
 *     Rt_h = sample_extract(BlindRotateGLWE(c_t; G_h, rotation_offset = rep / 2), 0)
 *   out = R(d-1)_0, key-switched in the reference's order; with the key switch first every digit is key-switched once,
 *   before its level, and the output has k N + 1 words.  lwe_out [batch][tables][io_words] decodes to
 *   T[sum_t x_t B^t].  Its padding bit is the one the reference's bootstrap of digit 0 leaves: that test vector
 *   answers x_0 = 0 under a negative phase error with -(B - T) Delta = T Delta - 2^31, the same message with the
 *   padding bit set; the upper levels (offset rep / 2) add nothing of the kind and pass it through.
 * The words equal the composition of tfhe_blind_rotate_batch, tfhe_sample_extract_batch, tfhe_pack_lwe_batch on the
 * materialised N-fold list, tfhe_blind_rotate_glwe_batch and tfhe_key_switch_batch; d = 1 equals tfhe_bootstrap_batch.
 * Cost: (B^d - 1) / (B - 1) rotations per (row, table) -- 85 for 8 bits at log_p = 2 -- and (B^(d-1) - 1) / (B - 1)
 * packings.  A level is one rotation call over all rows x tables x sub-tables and one packing call (in the chunks
 * the packing workspace holds, as tfhe_pack_lwe_batch_device); there is no host loop over rows, tables or sub-tables.
 *
 * Keys: the bootstrapping key and a packing key with from_dimension = k N made from the flattened GLWE key
 * (tfhe_generate_packing_key(ctx, flattened glwe_sk, k N, glwe_sk, ..)).  TFHE_ERR_NO_KEY when either is missing,
 * TFHE_ERR_INVALID_ARGUMENT when the packing key has another dimension, TFHE_ERR_UNSUPPORTED with a BMMP key.  A backend
 * that refuses the packing key (tfhe_load_packing_key: TFHE_ERR_EXACTNESS) cannot run it.
 *
 * Limits: 1 <= log_p < log2 N, d * log_p <= 16 (a table of at most 65,536 entries) and batch * tables * B^(d-1) < 2^31.
 * Workspace: tfhe_context_reserve_tree_lut(max_batch, max_digits, max_tables) reserves, for R = max_batch * max_tables *
 * B^(max_digits-1) level-0 rotations, R * [(n+1) + N + (k+1) N + (k N + 1)] + (R / B) * [(k N + 1) + (k+1) N] +
 * max_batch * (n+1) words: each rotation's copy of its row's digit and its test vector (the rotate kernels address sample
 * r's inputs at r * stride; copies instead of an index map keep them unchanged), the accumulators between the launches
 * of a segmented rotation, the two levels' results and the packed GLWEs.  At N = 1024, k = 1, n = 630, log_p = 2 that
 * is ~21 KiB per rotation: 1.3 GiB for 1,024 rows of 4 digits.  It covers every smaller call.  The _device form runs on
 * the context's stream and allocates nothing after it; a call beyond the reservation returns TFHE_ERR_INVALID_ARGUMENT
 * with the need in bytes.  digits is a host array of d device pointers.  The host form reserves for itself and blocks.
 *
 * Noise, in units of the 32-bit torus.  A level adds the rotation's
 *   s_br^2 = n * [ (k+1) l N (B_pbs^2/12 + 1/6) (sigma_glwe 2^32)^2 + (1 + k N / 2) 2^(2 ignored_bits_pbs) / 12 ]
 * and every level but the last the packing formula's with m = N and d = k N
 *   s_pk^2 = k N * l_ks * N * (B_ks^2/12 + 1/6) (sigma_glwe 2^32)^2 + (k N / 2) 2^(2 ignored_bits_ks) / 12
 * so the extraction R(d-1)_0 carries  sigma^2 = d * s_br^2 + (d-1) * s_pk^2,  independent of B^d; in the reference's
 * order the final key switch adds its own k N * l_ks (B_ks^2/12 + 1/6) (sigma_lwe 2^32)^2 + (k N / 2)
 * 2^(2 ignored_bits_ks) / 12.  A digit selects its block as long as its own phase error, after the modulus switch to
 * 2N, stays below half a block (2^32 / 4B), exactly as in a plain bootstrap. */
int tfhe_context_reserve_tree_lut(tfhe_context *ctx, size_t max_batch, size_t max_digits, size_t max_tables);
int tfhe_tree_lut_batch(tfhe_context *ctx, const uint32_t *const *digits, size_t d, size_t batch, const uint32_t *table,
                        size_t table_sets, size_t tables, uint32_t *lwe_out);
int tfhe_tree_lut_batch_device(tfhe_context *ctx, const uint32_t *const *digits, size_t d, size_t batch,
                               const uint32_t *table, size_t table_sets, size_t tables, uint32_t *lwe_out);

/* ---- ggsw.rs ------------------------------------------------------------------------------ */
/* external_product(): ggsw.rs:132-161.  ggsw [ggsw_count][(k+1)*l][k+1][N] with ggsw_count = 1
 * (one GGSW for the whole batch, the blind-rotation shape) or batch; glwe [batch][k+1][N]. */
int tfhe_external_product_batch(tfhe_context *ctx, const uint32_t *ggsw, size_t ggsw_count,
                                const uint32_t *glwe_in, size_t batch, uint32_t *glwe_out);
/* Device-pointer form used by the benchmark: `ggsw_prepared` (NTT domain, 8-byte words,
 * tfhe_prepared_ggsw_words() of them per GGSW) comes from tfhe_prepare_ggsw_device. */
int tfhe_prepared_ggsw_words(const tfhe_context *ctx, size_t *words);
int tfhe_prepare_ggsw_device(tfhe_context *ctx, const uint32_t *ggsw, size_t ggsw_count,
                             void *ggsw_prepared);
int tfhe_external_product_prepared_device(tfhe_context *ctx, const void *ggsw_prepared,
                                          size_t ggsw_count, const uint32_t *glwe_in, size_t batch,
                                          uint32_t *glwe_out);
/* cmux(): ggsw.rs:164-178.  Like the reference, ct1 is CLOBBERED with ct1 - ct0. */
int tfhe_cmux_batch(tfhe_context *ctx, const uint32_t *ggsw, size_t ggsw_count,
                    const uint32_t *ct0, uint32_t *ct1, size_t batch, uint32_t *glwe_out);
/* The same CMUX on the device with GGSW(s) prepared by tfhe_prepare_ggsw_device (ggsw_count = 1 or batch):
 * glwe_out[b] = ct0[b] + external_product(ggsw, ct1[b] - ct0[b]).  NOTHING is clobbered; glwe_out may not alias the
 * inputs.  Ordered on the context's stream, allocates nothing: safe under stream capture.  (It is a tree of one level
 * per sample in the tree kernel, one workgroup per sample: the CMUX path of the external-product kernel writes
 * ct1 - ct0 back, as the reference does, and is left as it is.) */
int tfhe_cmux_prepared_device(tfhe_context *ctx, const void *ggsw_prepared, size_t ggsw_count, const uint32_t *ct0,
                              const uint32_t *ct1, size_t batch, uint32_t *glwe_out);

/* ---- CMUX tree and encrypted table lookup (no reference counterpart; the reference stops at one cmux()) ----------
 * All arithmetic mod 2^32; ext = external_product (ggsw.rs:132-161) with the PBS decomposer in the context's alignment
 * mode; cmux(C, d0, d1) = d0 + ext(C, d1 - d0).
 *   Tree(C_0 .. C_{d-1}; L_0 .. L_{2^d - 1}):  L(0) = L,  L(i+1)_j = cmux(C_i, L(i)_{2j}, L(i)_{2j+1}),  result L(d)_0.
 *     With C_i a GGSW encryption of the bit b_i the tree selects leaf a = sum_i b_i 2^i: selector 0 is the least
 *     significant address bit and pairs neighbouring leaves.
 *   Lookup(C_0 .. C_{D-1}; T[0 .. 2^D)), T un-encoded values < 2^log_p, d_lo = min(D, log2 N), d_hi = D - d_lo:
 *     leaf h < 2^d_hi is the trivial GLWE (zero masks) whose body coefficient j is
 *     T[h 2^d_lo + j] << (32 - log_p - padding_bits) for j < 2^d_lo and 0 above;
 *     root = Tree(C_{d_lo} .. C_{D-1}; leaves) (leaf 0 if d_hi = 0);
 *     for i = 0 .. d_lo - 1 in this order: root = cmux(C_i, root, X^{-2^i} root)  (monomial index 2N - 2^i);
 *     out = sample_extract(root, 0): k N + 1 words under the flattened GLWE key, phase encode(T[a]) + noise.  The
 *     result feeds tfhe_key_switch_batch_device / tfhe_bootstrap_batch_device (KS-first order) unchanged.
 * No bootstrapping key is involved (nothing here returns TFHE_ERR_NO_KEY) and no new exactness rule applies: every
 * product has the (k+1) l rows and the base the context was admitted with.  A lookup is (2^d_hi - 1) + d_lo products.
 *
 * Noise: the selectors' errors and the decomposer's rounding add per product, so the error grows with D, not 2^D:
 *   sigma^2 <= D * [ (k+1) l N (B^2/12 + 1/6) (sigma_glwe 2^32)^2 + (1 + k N / 2) 2^(2 ignored_bits) / 12 ]
 * in units of the 32-bit torus, on top of the selected leaf's own noise (none for a clear table).
 *
 * Layouts.  selectors_prepared [queries][depth] prepared GGSWs (tfhe_prepare_ggsw_device over the raw
 * [queries][depth][(k+1) l][k+1][N]; selector i of a query is its address bit i).  Query q reads leaf set q, or the
 * one shared set (leaf_sets / table_sets = 1 or queries), once per table:
 *   leaves [leaf_sets][tables][2^depth][k+1][N]  ->  glwe_out [queries][tables][k+1][N]
 *   table  [table_sets][tables][2^depth] u32     ->  lwe_out  [queries][tables][k N + 1]
 * Values >= 2^log_p in a table are the caller's business (as with test vectors on the device).  Outputs may not alias
 * inputs.  Tree depth 1 .. 20, lookup depth 1 .. log2 N + 20.
 *
 * The _device forms run on the context's stream in a workspace sized by tfhe_context_reserve_lookup(max_trees,
 * max_tree_depth, max_lookup_bits) -- trees = queries * tables -- so that they never allocate or synchronise (safe under
 * stream capture; no second stream is used).  The reservation is a maximum: it covers every tfhe_cmux_tree_device call
 * of at most max_tree_depth levels and every tfhe_table_lookup_device call of at most max_lookup_bits address bits
 * (either may be 0: no such calls) over at most max_trees trees, under any subtree height, set before or after it.
 * It takes at most 3/4 * max_trees * 2^d * (k+1) * N * 4 bytes, d = max(max_tree_depth, max_lookup_bits - log2 N):
 * a lookup is sized by its OWN tree, so 1,024 lookups of 16 bits at N = 1024, k = 1 (d = 6) reserve 384 MiB, and
 * lookups of at most log2 N bits reserve nothing to speak of.  A call beyond the reservation returns
 * TFHE_ERR_INVALID_ARGUMENT with the reason.  The host forms take raw GGSWs and host arrays, upload, prepare the
 * selectors once, reserve for themselves and block.
 *
 * A call is ceil(d / h) launches, d the tree depth (d_hi for a lookup; one launch if d_hi = 0) and h the subtree
 * height one workgroup reduces.  The automatic h (the default) depends on d and on trees = queries * tables -- many
 * trees fill the chip with deep subtrees in one launch, a single tree goes out in short passes -- so the launches of
 * a call depend on its depth and its number of trees, but there is never a loop of launches over queries.
 * tfhe_context_set_lookup_subtree_height(h) fixes h (0: automatic again), and with it the launches whatever the
 * number of trees; the bits do not depend on it.  tfhe_debug_lookup_plan reports the height and the launches of a
 * tree of `depth` levels over `trees` trees (depth 0: a lookup without tree levels). */
int tfhe_context_reserve_lookup(tfhe_context *ctx, size_t max_trees, size_t max_tree_depth, size_t max_lookup_bits);
int tfhe_context_set_lookup_subtree_height(tfhe_context *ctx, unsigned height);
int tfhe_debug_lookup_plan(tfhe_context *ctx, size_t trees, size_t depth, unsigned *subtree_height, unsigned *launches);
int tfhe_cmux_tree_device(tfhe_context *ctx, const void *selectors_prepared, size_t queries, size_t depth,
                          const uint32_t *leaves, size_t leaf_sets, size_t tables, uint32_t *glwe_out);
int tfhe_cmux_tree(tfhe_context *ctx, const uint32_t *selectors, size_t queries, size_t depth, const uint32_t *leaves,
                   size_t leaf_sets, size_t tables, uint32_t *glwe_out);
int tfhe_table_lookup_device(tfhe_context *ctx, const void *selectors_prepared, size_t queries, size_t depth,
                             const uint32_t *table, size_t table_sets, size_t tables, uint32_t *lwe_out);
int tfhe_table_lookup(tfhe_context *ctx, const uint32_t *selectors, size_t queries, size_t depth, const uint32_t *table,
                      size_t table_sets, size_t tables, uint32_t *lwe_out);

/* ---- DEMUX tree and encrypted table update (no reference counterpart): the write port of the lookup ---------------
 * All arithmetic mod 2^32; ext and cmux as above.  The DEMUX tree is the transpose of Tree: it pushes ONE GLWE down the
 * selectors.
 *   Demux(C_0 .. C_{d-1}; x):  M(d)_0 = x
 *     for i = d-1 down to 0, j < 2^(d-1-i):
 *        M(i)_{2j+1} = ext(C_i, M(i+1)_j)
 *        M(i)_{2j}   = M(i+1)_j - M(i)_{2j+1}
 *     leaves M(0)_0 .. M(0)_{2^d - 1}
 *     Selector 0 is the least significant address bit and separates neighbouring leaves -- the convention of Tree, so
 *     Tree and Demux address the same leaf.  With C_i a GGSW encryption of the bit b_i, leaf a = sum_i b_i 2^i has the
 *     phase of x and every other leaf has phase 0.  Whatever the GGSWs hold, the leaves add up to x word for word.
 *   Write(C_0 .. C_{D-1}; V; table), d_lo = min(D, log2 N), d_hi = D - d_lo:
 *     x = V
 *     for i = 0 .. d_lo - 1 in this order: x = cmux(C_i, x, X^{2^i} x)          (monomial index 2^i)
 *     table[h] += Demux(C_{d_lo} .. C_{D-1}; x)_h   for h < 2^d_hi               (d_hi = 0: table[0] += x)
 *     V is a GLWE whose phase holds the encoded value in coefficient 0: a fresh encryption, or tfhe_pack_lwe_batch with
 *     per_group = 1 on a lookup's or a bootstrap's result.  Coefficients of V other than 0 move with it and wrap
 *     negacyclically: coefficient c of V lands on coefficient c + (a mod 2^d_lo) of leaf a >> d_lo, negated past N.
 *     The table is [2^d_hi][k+1][N] GLWEs with 2^d_lo entries per GLWE -- the leaf layout Lookup builds from a clear
 *     table: entry a is coefficient a mod 2^d_lo of leaf a >> d_lo.
 *   LookupGLWE(C_0 .. C_{D-1}; leaves [2^d_hi][k+1][N]):
 *     root = Tree(C_{d_lo} .. ; leaves) (leaf 0 if d_hi = 0); the rotation chain of Lookup; out = sample_extract(root, 0)
 *     -- the lookup over encrypted leaves instead of a clear table: what reads a written table back.
 * A DEMUX tree is 2^d - 1 products, a write d_lo + 2^d_hi - 1.  No bootstrapping key is involved (nothing here returns
 * TFHE_ERR_NO_KEY) and no new exactness rule applies.
 *
 * The write is ADDITIVE.  To replace entry a the caller writes new - old: old = tfhe_table_lookup_glwe at a, packed with
 * tfhe_pack_lwe_batch(per_group = 1), subtracted from the GLWE of the new value word by word, then written at a.  Several
 * queries into one shared table are a scatter-add: the leaves arrive as wrapping u32 atomic adds, which commute, so the
 * words do not depend on the order of arrival.
 *
 * Noise: every leaf, addressed or not, gains at most the lookup's per-product variance times the number of address bits,
 *   sigma^2 <= D * [ (k+1) l N (B^2/12 + 1/6) (sigma_glwe 2^32)^2 + (1 + k N / 2) 2^(2 ignored_bits) / 12 ]
 * on top of the value's own noise: W writes into one table followed by a read carry at most (W + 1) D of those terms on
 * every entry.
 *
 * Layouts.  selectors[_prepared] as for the lookup.  Query q writes leaf set q, or the one shared set (leaf_sets /
 * table_sets = 1 or queries), once per value / table:
 *   tfhe_demux_tree:        glwe_in [queries][values][k+1][N] -> leaves_out [leaf_sets][values][2^depth][k+1][N];
 *                           accumulate = 0 stores and needs leaf_sets == queries, accumulate = 1 adds into what is there
 *   tfhe_table_write:       values [queries][tables][k+1][N]  -> table_inout [table_sets][tables][2^d_hi][k+1][N], always adds
 *   tfhe_table_lookup_glwe: leaves [leaf_sets][tables][2^d_hi][k+1][N] -> lwe_out [queries][tables][k N + 1]
 * Outputs may not alias inputs.  Tree depth 1 .. 20, write and lookup depth 1 .. log2 N + 20.
 *
 * The _device forms of the first two run on the context's stream in a workspace sized by tfhe_context_reserve_demux(
 * max_trees, max_tree_depth, max_write_bits) -- trees = queries * values (tables) -- and never allocate or synchronise
 * (safe under stream capture; no second stream).  The reservation is a maximum: it covers every tfhe_demux_tree_device
 * call of at most max_tree_depth levels and every tfhe_table_write_device call of at most max_write_bits address bits
 * (either may be 0) over at most max_trees trees, under any subtree height.  It is the largest need over the heights
 * 1 .. d of  trees 2^(d-h) (h - 1)  parked nodes  +  trees 2^(d-h)  [ceil(d/h) >= 2]  +  trees 2^(d-2h)  [ceil(d/h) >= 3]
 * GLWEs of (k+1) N 4 bytes, d = max(max_tree_depth, max_write_bits - log2 N): at most 3/4 max_trees 2^d GLWEs.  A call
 * beyond the reservation returns TFHE_ERR_INVALID_ARGUMENT with the need in bytes and enqueues nothing.
 * tfhe_table_lookup_glwe_device runs in the lookup's workspace under tfhe_context_reserve_lookup's rule with
 * max_lookup_bits.  The host forms take raw GGSWs and host arrays, upload, prepare the selectors once, reserve for
 * themselves and block.
 *
 * A call is ceil(d / h) launches, top pass first: the lookup's plan walked in reverse, the top pass takes
 * d - (ceil(d / h) - 1) h levels and every later one h.  tfhe_context_set_demux_subtree_height(h) fixes h (0: automatic,
 * the lookup's rule); the bits do not depend on it.  tfhe_debug_demux_plan reports the height and the launches. */
int tfhe_context_reserve_demux(tfhe_context *ctx, size_t max_trees, size_t max_tree_depth, size_t max_write_bits);
int tfhe_context_set_demux_subtree_height(tfhe_context *ctx, unsigned height);
int tfhe_debug_demux_plan(tfhe_context *ctx, size_t trees, size_t depth, unsigned *subtree_height, unsigned *launches);
int tfhe_demux_tree_device(tfhe_context *ctx, const void *selectors_prepared, size_t queries, size_t depth,
                           const uint32_t *glwe_in, size_t values, uint32_t *leaves_out, size_t leaf_sets, int accumulate);
int tfhe_demux_tree(tfhe_context *ctx, const uint32_t *selectors, size_t queries, size_t depth, const uint32_t *glwe_in,
                    size_t values, uint32_t *leaves_out, size_t leaf_sets, int accumulate);
int tfhe_table_write_device(tfhe_context *ctx, const void *selectors_prepared, size_t queries, size_t depth,
                            const uint32_t *values, uint32_t *table_inout, size_t table_sets, size_t tables);
int tfhe_table_write(tfhe_context *ctx, const uint32_t *selectors, size_t queries, size_t depth, const uint32_t *values,
                     uint32_t *table_inout, size_t table_sets, size_t tables);
int tfhe_table_lookup_glwe_device(tfhe_context *ctx, const void *selectors_prepared, size_t queries, size_t depth,
                                  const uint32_t *leaves, size_t leaf_sets, size_t tables, uint32_t *lwe_out);
int tfhe_table_lookup_glwe(tfhe_context *ctx, const uint32_t *selectors, size_t queries, size_t depth,
                           const uint32_t *leaves, size_t leaf_sets, size_t tables, uint32_t *lwe_out);

/* ---- Encrypted branching programs (no reference counterpart): the lookup's CMUX over a DAG instead of a full tree -----
 * All arithmetic mod 2^32; ext and cmux as above.  A function of many input bits that has a small ordered binary
 * decision diagram -- a comparison, an equality, a range check, a carry chain -- costs one product per diagram node
 * (Chillotti, Gama, Georgieva, Izabachene 2017, section 5) where a table lookup costs 2^D / N.
 *
 * A PROGRAM over n_inputs selectors (GGSWs C_0 .. C_{n_inputs-1}, as for the lookup):
 *   terminals [n_terminals][N] clear message words; terminal t is the trivial GLWE with zero mask and body coefficient
 *     j = terminals[t][j] << tv_shift (the encoding of the lookup's leaves)
 *   nodes [n_nodes] of tfhe_program_node.  A reference r names terminal r if r < n_terminals, else node r - n_terminals.
 *     Node i may only reference terminals and nodes < i (topological order).  Its value is
 *       V_i = cmux(C_sel, R(lo), X^rot R(hi)),   sel < n_inputs,  rot in [0, 2N) a negacyclic monomial
 *     -- R(lo) where the selector holds 0, X^rot R(hi) where it holds 1.  A tree node has rot = 0; the lookup's rotation
 *     step i is lo = hi, rot = 2N - 2^i; the write's is lo = hi, rot = 2^i.
 *   outputs [n_outputs >= 1] references (a terminal is allowed: a constant function reduces to one)
 * Results: glwe_out [queries][n_outputs][k+1][N], and / or lwe_out [queries][n_outputs][k N + 1] = sample_extract(., 0)
 * under the flattened GLWE key -- what tfhe_key_switch_batch_device and tfhe_bootstrap_batch_device take (one of the two
 * may be NULL).  The program is clear and shared by all queries.  selectors[_prepared] [selector_sets][n_inputs] GGSWs,
 * selector_sets = queries (query q uses set q) or 1 (all queries share them); the host form takes raw GGSWs
 * [..][R][k+1][N] and host arrays, the device form prepared ones (tfhe_prepare_ggsw_device).  `nodes` and `outputs` are
 * HOST arrays in both forms (the program is clear: it is checked and planned on the host); `terminals`, the selectors
 * and the results are device memory in the device form.
 *
 * Noise: a CMUX adds one product's noise to the child it selects and the terminals are noise-free, so an output carries
 * at most the lookup's per-product variance times the DEPTH of the program (its longest path in products), not its size:
 *   sigma^2 <= depth * [ (k+1) l N (B^2/12 + 1/6) (sigma_glwe 2^32)^2 + (1 + k N / 2) 2^(2 ignored_bits) / 12 ]
 * No bootstrapping key is involved (nothing here returns TFHE_ERR_NO_KEY) and no new exactness rule applies: every
 * product has the (k+1) l rows and the base the context was admitted with.
 *
 * tfhe_cmux_program_device runs on the context's stream in the workspace of tfhe_context_reserve_program(max_queries,
 * max_nodes, max_outputs).  The need is host arithmetic:
 *   max_queries max_nodes (k+1) N 4 bytes   one GLWE per (query, node): the simple layout, no slot reuse
 *   + 4 (20 max_nodes + 4 max_outputs) bytes   four program images
 * and covers every call with at most that many queries, nodes and outputs under any split.  A call beyond it returns
 * TFHE_ERR_INVALID_ARGUMENT with its need in bytes and enqueues nothing.  The device form never allocates.  The FIRST
 * call with a given program uploads its image (the nodes ordered by dependency level) into one of the four image slots
 * of the workspace and synchronises the stream once; later calls with a program that is still resident (the four most
 * recently used) neither synchronise nor copy and are safe under stream capture.  A first use during a capture is
 * refused: run the program once before capturing.  An image used during a capture stays resident until the next
 * growing tfhe_context_reserve_program (which voids such graphs); if all four are held so, a fifth program is refused.
 * The host form reserves for itself, uploads, prepares the selectors once and blocks.
 *
 * Plan.  The host orders the nodes by dependency level (terminals 0, a node one more than its deeper operand).  With
 * one team per query the whole program is ONE launch: the throughput case.  With few queries the levels go out in
 * turn, the nodes of a level dealt to up to `parts` teams per query, consecutive levels of one team merged into one
 * launch; values that cross teams cross a launch boundary.  tfhe_context_set_program_split(parts) fixes parts (1: one
 * launch; 0: automatic, the cheapest of 1, 2, 4, .. under the lookup's cost model, whose per-launch cost is a guess,
 * not measured).  The output words do not depend on it.  tfhe_debug_program_plan reports the launches and the most
 * teams a launch gives one query for a program with one output.
 *
 * Refused with TFHE_ERR_INVALID_ARGUMENT and a message in tfhe_last_error: a forward or self reference, sel >=
 * n_inputs, rot >= 2N, an output reference out of range, n_outputs == 0, n_terminals == 0, selector_sets other than 1
 * or queries, NULL handles. */
typedef struct tfhe_program_node {
  uint32_t sel, lo, hi, rot;
} tfhe_program_node;
int tfhe_context_reserve_program(tfhe_context *ctx, size_t max_queries, size_t max_nodes, size_t max_outputs);
int tfhe_context_set_program_split(tfhe_context *ctx, unsigned parts);
int tfhe_debug_program_plan(tfhe_context *ctx, size_t queries, const tfhe_program_node *nodes, size_t n_nodes,
                            size_t n_terminals, unsigned *launches, unsigned *teams_per_query);
int tfhe_cmux_program_device(tfhe_context *ctx, const void *selectors_prepared, size_t queries, size_t n_inputs,
                             size_t selector_sets, const tfhe_program_node *nodes, size_t n_nodes, const uint32_t *terminals,
                             size_t n_terminals, const uint32_t *outputs, size_t n_outputs, uint32_t *glwe_out,
                             uint32_t *lwe_out);
int tfhe_cmux_program(tfhe_context *ctx, const uint32_t *selectors, size_t queries, size_t n_inputs, size_t selector_sets,
                      const tfhe_program_node *nodes, size_t n_nodes, const uint32_t *terminals, size_t n_terminals,
                      const uint32_t *outputs, size_t n_outputs, uint32_t *glwe_out, uint32_t *lwe_out);

/* ---- decomposer.rs / glwe.rs / utils.rs --------------------------------------------------- */
/* SignedDecomposer::decompose: decomposer.rs:42-80.  digits_out [count][levels], MSB first. */
int tfhe_decompose(tfhe_context *ctx, int which_decomposer, const uint32_t *values, size_t count,
                   uint32_t *digits_out);
/* decompose_glwe_ciphertext: glwe.rs:90-108.  glwe [batch][k+1][N] -> [batch][(k+1)*l][N] */
int tfhe_decompose_glwe_batch(tfhe_context *ctx, const uint32_t *glwe, size_t batch,
                              uint32_t *digits_out);
/* switch_modulus: utils.rs:23-33 */
int tfhe_switch_modulus(tfhe_context *ctx, const uint32_t *values, size_t count, uint32_t log_from,
                        uint32_t log_to, uint32_t *out);
/* &GlweCiphertext * &Monomial: glwe.rs:20-34, one monomial index per ciphertext */
int tfhe_glwe_mul_monomial_batch(tfhe_context *ctx, const uint32_t *glwe_in, size_t batch,
                                 const int64_t *monomial_index, uint32_t *glwe_out);

/* ---- lwe.rs ------------------------------------------------------------------------------- */
/* out = c0*ct0 + c1*ct1 over [batch][n+1] words (wrapping): `&a + &b` is (1, 1) (lwe.rs:9-15),
 * `&a * s` is (s, 0) with ct1 = NULL (lwe.rs:17-23), the gate input 2*ct1 + ct0 is (1, 2)
 * (boolean.rs:18).  `words_per_ct` lets the same call serve any LWE dimension. */
int tfhe_lwe_linear_batch(tfhe_context *ctx, uint32_t c0, const uint32_t *ct0, uint32_t c1,
                          const uint32_t *ct1, size_t batch, size_t words_per_ct, uint32_t *out);
int tfhe_lwe_linear_batch_device(tfhe_context *ctx, uint32_t c0, const uint32_t *ct0, uint32_t c1,
                                 const uint32_t *ct1, size_t batch, size_t words_per_ct,
                                 uint32_t *out);

/* ---- encrypted dense layers (no reference counterpart) --------------------------------------------
 * A clear integer matrix times a batch of LWE ciphertexts, and a whole layer (the product, then one programmable
 * bootstrap per output) in one call: the discretised neural-network layer of FHE-DiNN (Bourse, Minelli, Minihold,
 * Paillier 2018), the linear half of every "PBS as activation" pipeline.
 *
 *   Dense(W, bias; x):  out[q][o][c] = ( sum_{i<I} (u32)W[o][i] * x[q][i][c] )  mod 2^32      c < words_per_ct
 *                       out[q][o][words_per_ct-1] += bias[o]                                  (bias may be NULL)
 *
 * x [queries][I][words_per_ct]; W [O][I] int32, any value (two's complement is exact mod 2^32); bias [O] already
 * ENCODED words (as tfhe_lwe_encrypt_batch's plaintexts); out [queries][O][words_per_ct].  words_per_ct is explicit
 * as in tfhe_lwe_linear_batch: both boundary dimensions (n+1, k N + 1) and any other LWE size are served.  With I = 2
 * a row (c0, c1) of W is tfhe_lwe_linear_batch's c0*ct0 + c1*ct1.  Phases are linear: for any key,
 * phase(out[q][o]) = sum_i W[o][i] phase(x[q][i]) + bias[o] mod 2^32 exactly; a row of W multiplies the input
 * noise's variance by its squared Euclidean norm.
 *
 * Plan.  One launch of a tiled wrapping-u32 GEMM (csrc/lwe_dense.h): a workgroup owns one query, 32 outputs and 128
 * columns.  A call with too few tiles to fill the chip splits the inputs over several workgroups, whose partial sums
 * are added into the zeroed output (a memset node on the context's stream: the call stays capturable).
 * tfhe_context_set_dense_split(parts) fixes the split (1: none; 0: automatic); it is held to at most one split per
 * 16 inputs.  The output words never depend on it.  tfhe_debug_dense_plan reports the splits and the workgroups of
 * the launch.
 *
 * tfhe_dense_bootstrap_batch: lwe_out[q][o] = bootstrap(Dense(x)[q][o]; tv[o mod tv_count]), tv_count 1 or O, test
 * vectors [tv_count][N] un-encoded as for tfhe_bootstrap_batch.  x and lwe_out are at the context's boundary
 * dimension in either bootstrap order (n+1 words, or k N + 1 after tfhe_context_set_bootstrap_order(ctx, 1)); the
 * bootstraps are tfhe_bootstrap_batch's, [queries * O] of them.  The _device form runs in the workspace of
 * tfhe_context_reserve_dense(max_queries, max_outputs): the layer's pre-activations, one test vector per bootstrap
 * (per-neuron test vectors are copied out, one per (query, neuron)) and what a bootstrap of max_queries * max_outputs
 * rows needs: 4 max_queries max_outputs (words + N) bytes at the larger boundary dimension, plus tfhe_context_reserve
 * (max_queries * max_outputs).  Smaller calls fit.  After the reservation the _device form allocates nothing, enqueues
 * on the context's stream only and can be captured; a call beyond the reservation is refused and names its need in
 * bytes.  The host form reserves for itself.
 *
 * Refused with TFHE_ERR_INVALID_ARGUMENT and a message in tfhe_last_error: queries, I, O or words_per_ct of 0, NULL x /
 * W / out, out overlapping x, tv_count other than 1 or O, sizes whose tiles exceed one grid (queries *
 * ceil(words_per_ct / 128) >= 2^31, O > 32 * 65535, I >= 2^31).  The fused form: TFHE_ERR_NO_KEY without a
 * bootstrapping key, and TFHE_ERR_UNSUPPORTED wherever tfhe_bootstrap_batch is. */
int tfhe_context_reserve_dense(tfhe_context *ctx, size_t max_queries, size_t max_outputs);
int tfhe_context_set_dense_split(tfhe_context *ctx, unsigned parts);
int tfhe_debug_dense_plan(tfhe_context *ctx, size_t queries, size_t inputs, size_t outputs, size_t words_per_ct,
                          unsigned *splits, unsigned *workgroups);
int tfhe_lwe_dense_batch(tfhe_context *ctx, const uint32_t *x, size_t queries, size_t inputs, const int32_t *weights,
                         const uint32_t *bias, size_t outputs, size_t words_per_ct, uint32_t *out);
int tfhe_lwe_dense_batch_device(tfhe_context *ctx, const uint32_t *x, size_t queries, size_t inputs, const int32_t *weights,
                                const uint32_t *bias, size_t outputs, size_t words_per_ct, uint32_t *out);
int tfhe_dense_bootstrap_batch(tfhe_context *ctx, const uint32_t *x, size_t queries, size_t inputs, const int32_t *weights,
                               const uint32_t *bias, size_t outputs, const uint32_t *test_vector_poly, size_t tv_count,
                               uint32_t *lwe_out);
int tfhe_dense_bootstrap_batch_device(tfhe_context *ctx, const uint32_t *x, size_t queries, size_t inputs,
                                      const int32_t *weights, const uint32_t *bias, size_t outputs,
                                      const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);

/* ---- digit extraction: one LWE sum into bits or digits (no reference counterpart) ------------------------------------
 * The linear layers add ciphertexts exactly, so a sum of m inputs is log2 m bits wider than its inputs, while a
 * bootstrap resolves log_p bits, the tree LUT takes separate digits and the gates single bits.  This call takes the
 * wide value apart, least significant bit first, with one sign bootstrap per bit (FHE-DiNN's "sum, then split"; the
 * radix schemes' carry extraction).  Every bit is decided at bit 31, with a margin of 2^30, whatever its position.
 *
 * All arithmetic is mod 2^32.  lwe_in [batch][io_words] (io_words = n + 1, or k N + 1 with the key switch first) has
 * phase v 2^lsb + e.  The call extracts w = g d bits of v (g = digit_bits, d = digits), bit 0 first.  r_0 = lwe_in; for
 * j = 0 .. w-1, with t = j div g and i = j mod g:
 *   m_j     = min(lsb + j, out_lsb + i),   kappa_j = 2^(m_j - 1)
 *   s_j     = 2^(31-lsb-j) r_j                                          on every word
 *   o_j     = tfhe_bootstrap_glwe_batch(s_j; acc_in = (0, .., 0, kappa_j (1 + X + .. + X^(N-1))), acc_count = 1,
 *                                       rotation_offset = N / 2)        in the context's bootstrap order: phase
 *                                                                       +kappa_j for bit 0, -kappa_j for bit 1
 *   beta_j  = (0, .., 0, kappa_j) - o_j                                 phase b_j 2^(m_j)
 *   r_(j+1) = r_j - 2^(lsb+j-m_j) beta_j
 *   D_t    += 2^(out_lsb+i-m_j) beta_j                                  D_t starts at 0
 * digits_out is a host array of d pointers (device pointers in the _device form), each [batch][io_words]: digit t has
 * phase x_t 2^out_lsb, digit 0 least significant.  remainder_out [batch][io_words] may be NULL; it is r_w, the input
 * with the w extracted bits cleared: the bits of v above w stay in it (the carry).
 *
 * Limits: lsb >= 1 and out_lsb >= 1 (bit m_j - 1 holds the constant), lsb + w <= 32, out_lsb + g <= 32, 1 <= g, 1 <= d,
 * w <= 16.  Three settings cover the uses: g = 1, out_lsb = 32 - log_p - padding_bits gives gate-compatible bits;
 * g = log_p at the same out_lsb gives tree-LUT digits; lsb = out_lsb extracts a popcount of gate bits in place,
 * padding bit included.
 *
 * The words equal, byte for byte, the composition of tfhe_lwe_linear_batch, tfhe_bootstrap_glwe_batch and
 * tfhe_lwe_dense_batch with a bias for the constants.  Plan: the only host loop is over the w bits; a bit is one
 * bootstrap call and ONE elementwise launch (csrc/lwe_extract.h) that does step j's epilogue and step j+1's prologue
 * and writes the next constant accumulator: w bootstraps and w + 1 small launches per call, whatever the batch.
 *
 * Refused: TFHE_ERR_INVALID_ARGUMENT for a limit crossed, a NULL pointer, an empty batch, digit buffers that overlap
 * each other, remainder_out or (device form) lwe_in; TFHE_ERR_NO_KEY without a bootstrapping key; TFHE_ERR_UNSUPPORTED
 * with a BMMP key (the rotations start from a GLWE accumulator).
 *
 * Workspace: tfhe_context_reserve_extract(max_batch, max_digits) reserves, on top of tfhe_context_reserve(max_batch), r,
 * s, o and max_digits digit buffers of max_batch * (max(n, k N) + 1) words each (either bootstrap order fits) and one
 * accumulator of (k+1) N words.  After it the _device form allocates nothing, stays on the context's stream and can be
 * captured; it writes the digits to the caller's buffers and uses no digit buffer of the workspace.  A call beyond the
 * reservation returns TFHE_ERR_INVALID_ARGUMENT with the need in bytes.  The host form reserves for itself and blocks.
 *
 * Noise, in units of the 32-bit torus.  sigma_bs^2 is a bootstrap's output variance at the boundary: s_br^2 + s_ks^2 in
 * the reference's order and s_br^2 with the key switch first, with s_br^2 as in the tree LUT above and
 * s_ks^2 = k N l_ks (B_ks^2/12 + 1/6) (sigma_lwe 2^32)^2 + (k N / 2) 2^(2 ignored_bits_ks) / 12.  With
 * A_j = 2^(lsb+j-m_j) and sigma_in^2 the input's variance,
 *   Var(r_j) = sigma_in^2 + sum_{j' < j} A_j'^2 sigma_bs^2.
 * Bit j is decided correctly while the error the rotation sees stays below 2^30: 2^(31-lsb-j) |e(r_j)|, plus the
 * rotation's modulus-switch term of variance (1 + n/2) (2^32 / 2N)^2 / 12, plus -- with the key switch first -- the
 * key-switch term s_ks^2, which is added after the scaling and so not amplified.  Digit t carries
 *   sum_{i < g} 2^(2 (out_lsb+i-m_j)) sigma_bs^2,   j = t g + i,
 * independent of sigma_in.  (Where out_lsb + i <= lsb + j, the usual case, every factor is 1: g sigma_bs^2.)
 *
 * ---- wide LUT: any function of a d log_p-bit encrypted value ----
 * tfhe_wide_lut_batch is the extraction with g = log_p and out_lsb = 32 - log_p - padding_bits, remainder dropped,
 * followed by tfhe_tree_lut_batch_device on the d digits: one call, byte-identical to that composition.  table, table_sets,
 * tables and lwe_out [batch][tables][io_words] are the tree LUT's, with the tree LUT's limits, keys and refusals (the
 * packing key included) on top of the extraction's.  tfhe_context_reserve_wide_lut(max_batch, max_digits, max_tables) is
 * tfhe_context_reserve_extract(max_batch, max_digits) and tfhe_context_reserve_tree_lut(max_batch, max_digits,
 * max_tables); the device form keeps its digits in the extraction workspace.  Noise: the extraction's digits enter the
 * tree LUT with variance g sigma_bs^2; the output carries the tree LUT's own. */
int tfhe_context_reserve_extract(tfhe_context *ctx, size_t max_batch, size_t max_digits);
int tfhe_context_reserve_wide_lut(tfhe_context *ctx, size_t max_batch, size_t max_digits, size_t max_tables);
int tfhe_extract_digits_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned lsb, unsigned digit_bits,
                              unsigned digits, unsigned out_lsb, uint32_t *const *digits_out, uint32_t *remainder_out);
int tfhe_extract_digits_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned lsb,
                                     unsigned digit_bits, unsigned digits, unsigned out_lsb, uint32_t *const *digits_out,
                                     uint32_t *remainder_out);
int tfhe_wide_lut_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned lsb, size_t d,
                        const uint32_t *table, size_t table_sets, size_t tables, uint32_t *lwe_out);
int tfhe_wide_lut_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, unsigned lsb, size_t d,
                               const uint32_t *table, size_t table_sets, size_t tables, uint32_t *lwe_out);

/* ---- radix integers: blocks with carry space, log-depth carry propagation (no reference counterpart) ------------------
 * An encrypted integer is D blocks, each one LWE ciphertext with m message bits and m carry bits: log_p = 2 m, m >= 2,
 * P = 2^log_p, Bm = 2^m, Delta = 2^(32 - log_p - padding_bits), padding_bits >= 1.  A block of value v < P has phase
 * v Delta + e.  A radix integer is [batch][D][io_words] (io_words = n + 1, or k N + 1 with the key switch first), block 0
 * least significant; it is clean when every block is below Bm, and stands for sum_j v_j Bm^j mod Bm^D.  Blockwise sums
 * are plain wrapping adds of words (tfhe_lwe_linear_batch); these calls do what needs a bootstrap.  All arithmetic is
 * mod 2^32 on every word.
 *
 * Table lookup.  With rep = N / 2^(log_p + padding_bits - 1) >= 2 (N / P at padding_bits = 1: P <= N / 2), every lookup is
 *   LUT_T(x) = tfhe_bootstrap_glwe_batch(x; acc_in = (0, .., 0, sum_i T[i div rep] Delta X^i), acc_count = batch,
 *                                        rotation_offset = rep / 2)
 * one accumulator per rotation, in the context's bootstrap order (T is read for i div rep < P only).  The offset puts a
 * block's centre on the middle of its rep coefficients, so no table entry is negated; inputs must be below P (padding
 * bit clear).  Between two bootstrap levels there is ONE elementwise launch (csrc/radix.h): for every rotation of the
 * next level it forms  wa A[q][ia(j)] + wb B[q][ib(j)]  -- ia, ib a shifted or a fixed (broadcast) block index, an index
 * outside the operand reading the trivial zero ciphertext -- and writes that rotation's accumulator.  Shifts, weights and
 * table choices are kernel arguments computed on the host from (operation, D, level): nothing is uploaded per call.
 *
 * tfhe_radix_propagate_batch: blocks v_j <= P - 1 -> the clean integer of the same value mod Bm^D, in
 * 3 + ceil(log2(D - 1)) levels for D >= 2 (one for D = 1) instead of D:
 *   1. M_j = LUT_{x mod Bm}(v_j) and C_j = LUT_{x >> m}(v_j), one call of 2 D rotations per row (D = 1: M only, done)
 *   2. w_j = M_j + C_(j-1), C_(-1) = 0                                            (w_j <= 2 Bm - 2)
 *      S_0 = LUT_{[x >= Bm]}(w_0) -- complete, a carry in {0, 1};
 *      S_j = LUT_{0 none, 1 propagate (x = Bm - 1), 2 generate (x >= Bm)}(w_j), 1 <= j <= D - 2
 *   3. for r = 1, 2, 4, .. while r < D - 1: blocks j < r stay; for r <= j <= D - 2, x = 4 S_j + S_(j-r) (<= 10) and
 *        r <= j < 2 r:  S_j = LUT_{[hi = 2 or (hi = 1 and lo = 1)]}(x)    (the lower operand is complete: a carry)
 *        j >= 2 r:      S_j = LUT_{hi if hi != 1 else lo}(x)              with hi = x div 4, lo = x mod 4
 *   4. out_j = LUT_{x mod Bm}(w_j + S_(j-1)), S_(-1) = 0
 *
 * tfhe_radix_map_batch: one level,  out[q][j] = LUT_{tables[table_of_block[j]]}(wa a[q][ia(j)] + wb b[q][ib(j)])  for
 * j < blocks, with ia(j) = a_fixed if a_fixed >= 0 else j - a_shift (zero outside [0, a_blocks)), ib likewise; b may be
 * NULL (a univariate lookup).  a is [batch][a_blocks][io_words], b [batch][b_blocks][io_words], out [batch][blocks][io_words].
 * tables [table_count][P] holds un-encoded values below P, table_count <= 254 (a device pointer in the _device form,
 * where its values cannot be checked); table_of_block [blocks] is a host array in both forms.  That
 * wa v_a + wb v_b stays below P cannot be checked on ciphertexts: it is the caller's degree rule (clean operands with
 * (wa, wb) = (Bm, 1) keep it).  This is the primitive behind bitwise operations, partial products, shifts and select.
 *
 * tfhe_radix_compare_batch: clean a, b [batch][D][io_words] and a predicate -> out [batch][io_words], one block in {0, 1}:
 *   1. c_j = LUT_{0 equal, 1 less, 2 greater}(Bm a_j + b_j)
 *   2. while more than one code is left: pairs (hi, lo) of neighbours become LUT_{hi if hi != 0 else lo}(4 hi + lo); with
 *      an odd count the least significant code passes through (it is not bootstrapped) and the pairs start at code 1:
 *      ceil(log2 D) levels
 *   the predicate's table is composed into the last level's (level 1 for D = 1).
 *
 * The words of every call equal, byte for byte, the composition of tfhe_lwe_linear_batch (the sums) and
 * tfhe_bootstrap_glwe_batch on clear accumulators, one call per line above: the sums are exact, and the rotation kernels'
 * shapes agree bit for bit whatever the batch of a level.  (No line adds a constant, so tfhe_lwe_dense_batch's bias has
 * no part in it.)
 *
 * Limits and refusals.  TFHE_ERR_INVALID_ARGUMENT: log_p odd or below 4, padding_bits = 0, rep < 2, D = 0 or above 64, an
 * empty batch, 2 batch D above 2^31 - 1, a NULL pointer (b excepted), an output that overlaps an input other than exactly
 * in place, a table index out of range, (host form) a table value >= P, an unknown predicate.  TFHE_ERR_NO_KEY without a
 * bootstrapping key; TFHE_ERR_UNSUPPORTED with a BMMP key (the rotations start from a GLWE accumulator).  Nothing is
 * enqueued by a refused call.
 *
 * Workspace: tfhe_context_reserve_radix(max_batch, max_blocks) reserves tfhe_context_reserve(R), R = 2 max_batch max_blocks
 * rotations, and on top of it, with W = max(n, k N) + 1 (either bootstrap order fits):
 *   6 roundup4(max_batch max_blocks W) + R (k+1) N   words of 4 bytes
 * -- a level's inputs and level 1's results (R rows each), the sums w and the states s (R / 2 rows each), and R
 * accumulators -- plus the 20 fixed tables of P words, written once (that call may synchronise).  After it the _device
 * forms allocate nothing, stay on the context's stream and can be captured.  A call beyond the reservation returns
 * TFHE_ERR_INVALID_ARGUMENT with the need in bytes.  The host forms reserve for themselves and block.
 *
 * Noise, in units of the 32-bit torus, with sigma_bs^2 a bootstrap's output variance at the boundary exactly as the digit
 * extraction above defines it.  A level's input is a combination with weights (wa, wb) of bootstrap outputs: variance
 * (wa^2 + wb^2) sigma_bs^2, the weights at most (4, 1) inside propagate and compare, (Bm, 1) for a bivariate map on fresh
 * blocks; level 1 sees the caller's variance.  A block is decided correctly while that error, plus the rotation's
 * modulus-switch term of variance (1 + n/2) (2^32 / 2N)^2 / 12, plus -- with the key switch first -- the key-switch term
 * s_ks^2, stays below half a block, Delta / 2 = 2^32 / (2^(padding_bits + 1) P). */
#define TFHE_RADIX_EQ 0
#define TFHE_RADIX_NE 1
#define TFHE_RADIX_LT 2
#define TFHE_RADIX_LE 3
#define TFHE_RADIX_GT 4
#define TFHE_RADIX_GE 5
int tfhe_context_reserve_radix(tfhe_context *ctx, size_t max_batch, size_t max_blocks);
int tfhe_radix_propagate_batch(tfhe_context *ctx, const uint32_t *blocks_in, size_t batch, size_t blocks,
                               uint32_t *blocks_out);
int tfhe_radix_propagate_batch_device(tfhe_context *ctx, const uint32_t *blocks_in, size_t batch, size_t blocks,
                                      uint32_t *blocks_out);
int tfhe_radix_map_batch(tfhe_context *ctx, const uint32_t *a, size_t a_blocks, uint32_t wa, int32_t a_shift,
                         int32_t a_fixed, const uint32_t *b, size_t b_blocks, uint32_t wb, int32_t b_shift,
                         int32_t b_fixed, size_t batch, size_t blocks, const uint32_t *tables, size_t table_count,
                         const uint32_t *table_of_block, uint32_t *out);
int tfhe_radix_map_batch_device(tfhe_context *ctx, const uint32_t *a, size_t a_blocks, uint32_t wa, int32_t a_shift,
                                int32_t a_fixed, const uint32_t *b, size_t b_blocks, uint32_t wb, int32_t b_shift,
                                int32_t b_fixed, size_t batch, size_t blocks, const uint32_t *tables, size_t table_count,
                                const uint32_t *table_of_block, uint32_t *out);
int tfhe_radix_compare_batch(tfhe_context *ctx, const uint32_t *a, const uint32_t *b, size_t batch, size_t blocks,
                             unsigned predicate, uint32_t *out);
int tfhe_radix_compare_batch_device(tfhe_context *ctx, const uint32_t *a, const uint32_t *b, size_t batch, size_t blocks,
                                    unsigned predicate, uint32_t *out);

/* ---- multi-value bootstrapping: several tables from one blind rotation (no reference counterpart) --------------------
 * Several functions of ONE ciphertext cost one rotation, not one each (Carpov, Izabachene, Mollimard 2019): rotate a
 * table-independent accumulator, then multiply it by a small clear polynomial per table.  Nothing is packed into spare
 * bits of the input; the modulus switch and the rotation are the bootstrap's own.  The price is output noise, below.
 *
 * Let B = 2^log_p, rep = N / B >= 2 (log_p < log2 N), kappa = 2^(31 - log_p - padding_bits) (log_p + padding_bits <= 31).
 * For a lookup table T[0 .. B) let h = (T[0] != 0 ? B - T[0] : 0), the value construct_test_from_lut writes in the place
 * of T[0] on the half block that wraps to the top of the test vector (test_vector.rs:38-67).  With terms = B + 1:
 *   m = 0          position p_0 = 0                       D[0] = T[0] + h
 *   m = 1 .. B-1   position p_m = rep/2 + (m-1) rep       D[m] = T[m] - T[m-1]
 *   m = B          position p_B = N - rep/2               D[B] = h - T[B-1]
 * in int32 (two's complement wraps exactly mod 2^32).  sum_m D[m] X^(p_m) = (1 - X) tv(X) in Z[X]/(X^N + 1) with
 * tv = construct_test_from_lut(T), and (1 + X + .. + X^(N-1)) (1 - X) = 2, so kappa (1 + .. + X^(N-1)) (1 - X) tv =
 * tv << (32 - log_p - padding_bits), word for word mod 2^32.
 *
 * tfhe_multi_value_bootstrap_batch(lwe_in [batch][io_words], luts [lut_sets][tables][B] un-encoded values below B,
 * lut_sets 1 or batch) -> lwe_out [batch][tables][io_words]:
 *   1. A_q = tfhe_blind_rotate_glwe_batch(lwe_in[q]; acc_in = (0, .., 0, kappa (1 + X + .. + X^(N-1))), acc_count = 1,
 *      rotation_offset = 0); with the key switch first, lwe_in is key-switched before, as in a bootstrap.
 *   2. out[q][t] = D_t[0] SE_0(A_q) - sum_{m >= 1} D_t[m] SE_(N - p_m)(A_q), SE_j the words of
 *      tfhe_sample_extract_batch at index j, wrapping u32 on the k N + 1 words (coefficient 0 of X^p A is -A[N - p] for
 *      0 < p < N).  This is tfhe_glwe_sparse_extract_batch with positions p and coefficients D.
 *   3. In the reference's order every out[q][t] is key-switched, AFTER the combination: the key switch's noise is not
 *      amplified.
 * The words equal that composition of public entry points byte for byte.  Under noise-free keys that ignore no bits the
 * phase of lwe_out[q][t] is exactly the phase tfhe_bootstrap_batch gives with construct_test_from_lut(T_t), the
 * padding-bit case included.
 *
 * tfhe_glwe_sparse_extract_batch(glwe [batch][k+1][N], positions [terms] in HOST memory in both forms, distinct, each
 * below N; coeffs int32 [sets][tables][terms], sets 1 or batch) -> lwe_out [batch][tables][k N + 1] is step 2 for any
 * sparse clear polynomials sum_m c[m] X^(p_m): out[q][t] = sum_m c[set][t][m] (p_m = 0 ? SE_0(A_q) : -SE_(N - p_m)(A_q)),
 * the LWE ciphertext of coefficient 0 of the product.  No transform, no exactness rule: the same words in every backend.
 *
 * Plan (csrc/multi_value.h): one workgroup per (input, run of tables) stages A_q in LDS once and writes whole rows; with
 * few inputs the tables are dealt over the grid.  The lookup tables become coefficient rows in one small launch.
 *
 * tfhe_context_set_tree_lut_level0(ctx, 1): level 0 of tfhe_tree_lut_batch[_device] (and of tfhe_wide_lut_batch) becomes
 * ONE rotation per row and one step-2 launch over the tables * B^(d-1) sub-tables, whose table layout
 * [table_sets][tables * B^(d-1)][B] is already luts'; the results keep the order (row, table, h) the packing of level 1
 * expects.  Levels >= 1, the packing and the final key switch do not change; the call fits the workspace
 * tfhe_context_reserve_tree_lut reserves.  Rotations per (row, table): 5 -> 2 at d = 2, 21 -> 6 at d = 3, 85 -> 22 at
 * d = 4 (B = 4).  0 (the default): today's words, today's launches.  The setter allocates the constant accumulator.
 *
 * Refused: TFHE_ERR_INVALID_ARGUMENT for a NULL pointer, an empty batch, no table, sets / lut_sets not 1 or batch,
 * batch * tables >= 2^31, a position >= N or repeated, terms outside [1, N], log_p + padding_bits > 31, log_p >= log2 N;
 * TFHE_ERR_NO_KEY without a bootstrapping key; TFHE_ERR_UNSUPPORTED with a BMMP key (the shared rotation starts from a
 * GLWE accumulator).
 *
 * Workspace: tfhe_context_reserve_multi_value(max_batch, max_tables) reserves the key-switched inputs
 * [max_batch][n + 1], the rotated accumulators [max_batch][k+1][N], the coefficients [max_batch][max_tables][B + 1] and
 * the combinations [max_batch][max_tables][k N + 1] (either bootstrap order fits), and the constants.  After it the
 * _device forms allocate nothing, stay on the context's stream and can be captured (a caller's positions travel as
 * kernel arguments).  A call beyond the reservation returns TFHE_ERR_INVALID_ARGUMENT with the need in bytes.  The host
 * forms reserve for themselves and block.
 *
 * Noise, in units of the 32-bit torus.  The rotated accumulator carries s_br^2, the tree LUT's formula above; it does
 * not depend on the table.  out_t carries ||D_t||_2^2 s_br^2, plus s_ks^2 in the reference's order (un-amplified: the
 * key switch comes last), with ||D_t||_2^2 <= B^2 + B (B - 1)^2.  With ignored decomposer bits the rounding term scales
 * with ||D_t||_1.  A tree with the switch on carries ||D||_2^2 s_br^2 + (d - 1) s_br^2 + (d - 1) s_pk^2 (+ s_ks^2),
 * ||D||_2^2 the largest over its sub-tables.  A result decodes while 8 sigma stays below half a step,
 * 2^(31 - log_p - padding_bits). */
int tfhe_context_reserve_multi_value(tfhe_context *ctx, size_t max_batch, size_t max_tables);
int tfhe_context_set_tree_lut_level0(tfhe_context *ctx, int multi_value);
int tfhe_glwe_sparse_extract_batch(tfhe_context *ctx, const uint32_t *glwe, size_t batch, const uint32_t *positions,
                                   size_t terms, const int32_t *coeffs, size_t sets, size_t tables, uint32_t *lwe_out);
int tfhe_glwe_sparse_extract_batch_device(tfhe_context *ctx, const uint32_t *glwe, size_t batch, const uint32_t *positions,
                                          size_t terms, const int32_t *coeffs, size_t sets, size_t tables,
                                          uint32_t *lwe_out);
int tfhe_multi_value_bootstrap_batch(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, const uint32_t *luts,
                                     size_t lut_sets, size_t tables, uint32_t *lwe_out);
int tfhe_multi_value_bootstrap_batch_device(tfhe_context *ctx, const uint32_t *lwe_in, size_t batch, const uint32_t *luts,
                                            size_t lut_sets, size_t tables, uint32_t *lwe_out);

/* ---- encrypted convolutions (no reference counterpart) --------------------------------------------
 * A matrix of clear polynomials with small integer coefficients times a batch of GLWE ciphertexts: the general leveled
 * operation on packed ciphertexts that needs no GGSW (tfhe_glwe_mul_monomial_batch is the case of one weight +-X^r).
 *
 *   Conv(W, bias; x):  out[q][o][p] = sum_{c<C} W[o][c](X) * x[q][c][p](X)   in Z_{2^32}[X] / (X^N + 1),   p = 0..k
 *                      out[q][o][k] += bias[o]                                                  (bias may be NULL)
 *
 * x [queries][C][k+1][N]: C GLWE ciphertexts per query, one per input channel; W [O][C][N] int32 weight polynomials;
 * bias [O][N] already ENCODED words; out [queries][O][k+1][N].  The arithmetic is wrapping 32-bit with the negacyclic
 * wrap, so for any GLWE key phase(out[q][o]) = sum_c W[o][c] * phase(x[q][c]) + bias[o] mod 2^32 exactly, noise
 * included: per output coefficient the noise variance is sum_c ||W[o][c]||_2^2 times the inputs'.  An H x W image packed
 * row-major into one GLWE times a kernel whose tap (dy, dx) sits at coefficient (kh-1-dy) W + (kw-1-dx) carries output
 * pixel (y, x) of the "valid" correlation at coefficient (y+kh-1) W + (x+kw-1); the sum over c is a convolution layer
 * (nn.py::Conv2d).  The same product is the inner product of a packed query with a clear database column.
 *
 * Weights are prepared once (tfhe_prepare_poly_weights: their forward transforms, on the device; this one call
 * synchronises, and it takes HOST weights because the admission needs max |w|).  weight_bits is the smallest b with
 * every |w| <= 2^b, and the backend must admit some number of rows R >= 1 at base 2^weight_bits under its exactness
 * rule for R rows (the complex transform: FftField::error_bound(log N, R, weight_bits) < 1/4; the prime fields: log2 R +
 * log N + weight_bits + key_bits < exact_bits; each field's largest row count and small operand): rows_per_pass is the
 * largest such R.  If there is none the call returns TFHE_ERR_EXACTNESS with the reason in tfhe_last_error.  At most
 * rows_per_pass channels are summed in the transform domain; the passes are lifted to u32 on their own and meet in
 * wrapping additions, so the words do not depend on rows_per_pass.  Splitting larger weights into limbs is out of
 * scope (the noise grows with ||w||_2 anyway).  A weight set belongs to the device, backend and ring degree of the
 * context that prepared it, outlives that context's calls, and is destroyed by the caller (NULL is allowed).
 *
 * Plan.  Per call the queries * C * (k+1) ciphertext polynomials are transformed into the workspace of
 * tfhe_context_reserve_glwe_conv(max_queries, max_channels) (8 * parts * N bytes each, parts = 1 or 2 spectra by
 * backend: host arithmetic only), then one launch of queries * O teams multiplies, accumulates, transforms back and
 * lifts (csrc/glwe_conv.h).  tfhe_context_set_glwe_conv_rows(rows) fixes the channels per pass (0: automatic, the
 * admitted maximum); a value above what the backend admits for any weights is refused there, one above a weight set's
 * rows_per_pass at the call.  tfhe_debug_glwe_conv_plan reports rows per pass, passes and teams of a call.
 *
 * The _device forms enqueue on the context's stream only, allocate nothing after the reserve call and can be
 * captured; a call beyond the reservation is refused and names its need in bytes.  The host forms reserve for
 * themselves.  Refused with TFHE_ERR_INVALID_ARGUMENT and a message in tfhe_last_error: NULL x / weights / out,
 * queries, outputs or channels of 0, out overlapping x, weights of another context's device, backend or ring,
 * queries * O or queries * C * (k+1) >= 2^31.
 *
 * tfhe_sample_extract_indices: lwe_out[b][i] = tfhe_sample_extract_batch(glwe[b], indices[i]) for i < count -- a
 * convolution layer reads hundreds of coefficients per GLWE.  glwe [batch][k+1][N], lwe_out [batch][count][k N + 1].
 * The host form refuses an index >= N; the _device form takes indices on the device and reads them mod N. */
typedef struct tfhe_poly_weights tfhe_poly_weights;
int tfhe_prepare_poly_weights(tfhe_context *ctx, const int32_t *weights, size_t outputs, size_t channels,
                              tfhe_poly_weights **out);
void tfhe_poly_weights_destroy(tfhe_poly_weights *weights);
int tfhe_poly_weights_info(const tfhe_poly_weights *weights, size_t *outputs, size_t *channels, unsigned *weight_bits,
                           unsigned *rows_per_pass);
int tfhe_context_reserve_glwe_conv(tfhe_context *ctx, size_t max_queries, size_t max_channels);
int tfhe_context_set_glwe_conv_rows(tfhe_context *ctx, unsigned rows);
int tfhe_debug_glwe_conv_plan(tfhe_context *ctx, const tfhe_poly_weights *weights, size_t queries, unsigned *rows_per_pass,
                              unsigned *passes, unsigned *teams);
int tfhe_glwe_conv_batch(tfhe_context *ctx, const uint32_t *x, size_t queries, const tfhe_poly_weights *weights,
                         const uint32_t *bias, uint32_t *out);
int tfhe_glwe_conv_batch_device(tfhe_context *ctx, const uint32_t *x, size_t queries, const tfhe_poly_weights *weights,
                                const uint32_t *bias, uint32_t *out);
int tfhe_sample_extract_indices(tfhe_context *ctx, const uint32_t *glwe, size_t batch, const uint32_t *indices, size_t count,
                                uint32_t *lwe_out);
int tfhe_sample_extract_indices_device(tfhe_context *ctx, const uint32_t *glwe, size_t batch, const uint32_t *indices,
                                       size_t count, uint32_t *lwe_out);

/* ---- test_vector.rs / boolean.rs ---------------------------------------------------------- */
/* construct_test_from_lut: test_vector.rs:38-67 (host-side, no GPU).  out [N] */
int tfhe_construct_test_from_lut(const tfhe_params *params, const uint32_t *lut, size_t lut_len,
                                 uint32_t *out);
/* construct_test_vector_boolean: test_vector.rs:5-20 with the closure given as its truth table
 * truth[(lhs << 1) | rhs] */
int tfhe_construct_test_vector_boolean(const tfhe_params *params, const uint32_t truth[4],
                                       uint32_t *out);
/* and()/or(): boolean.rs:9-53 generalised over the closure: out = bootstrap(2*ct1 + ct0) with the
 * closure's test vector.  AND = {0,0,0,1}, OR = {0,1,1,1}, NAND = {1,1,1,0}, XOR = {0,1,1,0}.
 *
 * The table cache (tfhe_gate_batch* and tfhe_lut_gate_batch*).  The context keeps the device test vector of
 * every truth table it has seen, keyed on the table's length and entries: 64 tables, the least recently used
 * one replaced by the 65th.  The FIRST use of a table (and the first after it was replaced) builds the test
 * vector on the host and uploads it, which synchronises the context's stream; a call with a cached table
 * enqueues only.  An upload cannot happen while the stream is capturing: there the first use of a table is
 * refused with TFHE_ERR_INVALID_ARGUMENT and nothing enqueued (the capture stays valid), so run every gate
 * of a graph once eagerly before capturing it.
 * Guarantee for captured graphs: a table looked up during a capture is pinned for the life of the context.
 * Pinned tables are never replaced and do not count towards the 64 (each costs 4 N bytes of device memory),
 * so the test vector a captured graph reads is never rewritten with another table, however many other
 * tables go through the cache between replays. */
int tfhe_gate_batch(tfhe_context *ctx, const uint32_t truth[4], const uint32_t *ct0,
                    const uint32_t *ct1, size_t batch, uint32_t *lwe_out);
int tfhe_gate_batch_device(tfhe_context *ctx, const uint32_t truth[4], const uint32_t *ct0,
                           const uint32_t *ct1, size_t batch, uint32_t *lwe_out);
/* Gates of m inputs by the same recipe (notes/Boolean Gates.md:2-11): one PBS of
 * c_in = sum_i 2^i * cts[i] (cts[0] = rightmost / least significant input) with the test vector of
 * lut[x] = truth[x mod 2^m]; truth has 2^m entries < 2^log_p; 1 <= m <= min(log_p, 8) -- three-input
 * gates need a context with log_p >= 3.  cts is an array of m pointers to [batch][n+1]. */
int tfhe_lut_gate_batch(tfhe_context *ctx, const uint32_t *truth, uint32_t inputs,
                        const uint32_t *const *cts, size_t batch, uint32_t *lwe_out);
int tfhe_lut_gate_batch_device(tfhe_context *ctx, const uint32_t *truth, uint32_t inputs,
                               const uint32_t *const *cts, size_t batch, uint32_t *lwe_out);
/* NOT without a bootstrap: (-a, enc(1) - b) with enc(1) = 1 << (32 - log_p - padding_bits) */
int tfhe_lwe_not_batch(tfhe_context *ctx, const uint32_t *ct, size_t batch, uint32_t *lwe_out);
int tfhe_lwe_not_batch_device(tfhe_context *ctx, const uint32_t *ct, size_t batch,
                              uint32_t *lwe_out);

/* ---- encryption side: keygen / encrypt / decrypt --------------------------------
 * The reference draws its randomness from the caller's `rng: &mut R` (uniform masks with
 * sample_uniform_array, errors with sample_gaussian_array); the draws stay with the caller here too:
 * every in/out buffer arrives PRE-FILLED -- mask words hold the uniform samples, the body word /
 * body polynomial holds the error sample(s) -- and the call turns it into the ciphertext by adding
 * the <mask, key> term (and the message).  That makes each call a pure function of its arguments,
 * bit-comparable with the oracle.  Secret keys are host pointers and must be binary (sample_binary,
 * the only kind the reference generates): other values are refused with TFHE_ERR_INVALID_ARGUMENT. */
/* encrypt_glwe_zero glwe.rs:190-209: glwe [count][k+1][N] in/out, glwe_sk [k][N];
 * body += sum_i a_i * s_i.  encrypt_glwe_plaintext (:211-230) = error + message in the body. */
int tfhe_glwe_encrypt_zero_batch(tfhe_context *ctx, const uint32_t *glwe_sk, uint32_t *glwe,
                                 size_t count);
int tfhe_glwe_encrypt_zero_batch_device(tfhe_context *ctx, const uint32_t *glwe_sk, uint32_t *glwe,
                                        size_t count);
/* decrypt_glwe_ciphertext glwe.rs:245-265: plaintext_out [count][N] = body - sum_i a_i * s_i */
int tfhe_glwe_decrypt_batch(tfhe_context *ctx, const uint32_t *glwe_sk, const uint32_t *glwe,
                            size_t count, uint32_t *plaintext_out);
/* encrypt_ggsw_plaintext ggsw.rs:76-130 for `count` messages: ggsw [count][(k+1)l][k+1][N] in/out
 * (every row pre-filled like a GLWE above), messages [count] */
int tfhe_ggsw_encrypt_batch(tfhe_context *ctx, const uint32_t *glwe_sk, const uint32_t *messages,
                            uint32_t *ggsw, size_t count);
int tfhe_ggsw_encrypt_batch_device(tfhe_context *ctx, const uint32_t *glwe_sk,
                                   const uint32_t *messages /* host */, uint32_t *ggsw, size_t count);
/* encrypt_lwe_plaintext lwe.rs:138-160 (encrypt_lwe_zero :117-136 with plaintexts == NULL):
 * lwe [batch][dimension+1] in/out, b += <a, s> + plaintexts[i] (already encoded, lwe.rs:81-90) */
int tfhe_lwe_encrypt_batch(tfhe_context *ctx, const uint32_t *lwe_sk, size_t dimension,
                           const uint32_t *plaintexts, uint32_t *lwe, size_t batch);
int tfhe_lwe_encrypt_batch_device(tfhe_context *ctx, const uint32_t *lwe_sk, size_t dimension,
                                  const uint32_t *plaintexts /* device or NULL */, uint32_t *lwe,
                                  size_t batch);
/* decrypt_lwe lwe.rs:162-173: plaintext_out [batch] = b - <a, s> (still encoded; decode = shift) */
int tfhe_lwe_decrypt_batch(tfhe_context *ctx, const uint32_t *lwe_sk, size_t dimension,
                           const uint32_t *lwe, size_t batch, uint32_t *plaintext_out);
int tfhe_lwe_decrypt_batch_device(tfhe_context *ctx, const uint32_t *lwe_sk, size_t dimension,
                                  const uint32_t *lwe, size_t batch, uint32_t *plaintext_out);
/* KeySwitchingKey::generate_ksk key_switching.rs:20-60: ksk [from_dimension*l_ks][to_dimension+1]
 * in/out pre-filled row by row like an LWE; from_sk [from_dimension], to_sk [to_dimension]; uses
 * the context's ks_decomposer */
int tfhe_generate_ksk(tfhe_context *ctx, const uint32_t *from_sk, size_t from_dimension,
                      const uint32_t *to_sk, size_t to_dimension, uint32_t *ksk);
/* bootstrapping_key_gen bootstrapping.rs:23-56: bsk [n][(k+1)l][k+1][N] and ksk [kN*l_ks][n+1]
 * in/out, pre-filled; lwe_sk [n], glwe_sk [k][N] (the KSK goes from the flattened GLWE key
 * lwe.rs:62-73 to lwe_sk).  `load` != 0 also installs the result as the context's key, without a
 * round trip through the host for the _device form. */
int tfhe_bootstrapping_key_gen(tfhe_context *ctx, const uint32_t *lwe_sk, const uint32_t *glwe_sk,
                               uint32_t *bsk, uint32_t *ksk, int load);
int tfhe_bootstrapping_key_gen_device(tfhe_context *ctx, const uint32_t *lwe_sk,
                                      const uint32_t *glwe_sk, uint32_t *bsk, uint32_t *ksk,
                                      int load);
/* The same for the unrolled blind rotation: bsk_bmmp [n/2][3][(k+1)*l][k+1][N] pre-filled like bsk; the three
 * GGSWs of pair j encrypt s_2j s_2j+1, s_2j (1 - s_2j+1), s_2j+1 (1 - s_2j)
 * (notes/BMMP Bootstrapping.md:22-24).  `load` installs the key (BMMP mode). */
int tfhe_bootstrapping_key_gen_bmmp(tfhe_context *ctx, const uint32_t *lwe_sk, const uint32_t *glwe_sk,
                                    uint32_t *bsk_bmmp, uint32_t *ksk, int load);
int tfhe_bootstrapping_key_gen_bmmp_device(tfhe_context *ctx, const uint32_t *lwe_sk,
                                           const uint32_t *glwe_sk, uint32_t *bsk_bmmp, uint32_t *ksk,
                                           int load);

/* ---- seeded ciphertexts and compressed keys (no reference counterpart) ------------------------------------------------
 * The uniform mask words of a fresh ciphertext or of a key are public randomness; only the bodies depend on the key, the
 * message and the noise.  A seeded object is a short seed plus the bodies, and the masks are re-derived here by a public,
 * deterministic expansion function.  Secrets and errors are still the caller's draws (see "encryption side" above): this
 * is not a random number generator for them.
 *
 * The generator.  G(seed, domain)[w], for w < TFHE_SEED_MAX_WORDS = 2^36, is word (w mod 16) of the ChaCha20 block
 * function of RFC 8439 section 2.3 (20 rounds) with
 *   key           = seed.key, as eight little-endian words,
 *   block counter = w div 16 (below 2^32),
 *   nonce words   = (domain, low half of seed.stream, high half of seed.stream),
 *   output        = the sixteen state words after the final addition, as uint32_t.
 * With key bytes 00..1f, domain = 0x09000000 and stream = 0x4a000000 the words 16..31 are the RFC's own vector (2.3.2):
 * e4e7f110 15593bd1 ...  4e3c50a2.  tfhe_seed_words is the definition: host code, no context, no GPU.
 *
 * Layouts.  Seeded LWE rows are bodies[rows] plus a dimension d:
 *   full[r][j] = G(seed, TFHE_SEED_DOMAIN_LWE)[(first_row + r) d + j] for j < d,  full[r][d] = bodies[r]
 * (LWE batches of either boundary dimension, the key-switching key).  Seeded GLWE rows are bodies[rows][N]:
 *   full[r][i][j] = G(seed, TFHE_SEED_DOMAIN_GLWE)[((first_row + r) k + i) N + j] for i < k,  full[r][k][.] = bodies[r][.]
 * (GLWE, GGSW, the bootstrapping key -- ordinary, BMMP, multi-bit --, the packing key, the GLWE switch keys: all rows of
 * [k+1][N]).  first_row: a shard or a chunk expands rows [first_row, first_row + rows) of a larger object without the
 * rest.
 *
 * GGSWs.  Row (i, level) of a GGSW in the reference's form (ggsw.rs:76-130) is an encryption of zero plus m g_level on
 * polynomial i, and for i < k that is a MASK polynomial: a' = a + m g_level e_i.  a' is as uniform as a, so the seeded form
 * takes a' = G(seed) and the body says the rest: b = <a', s> + e - m g_level s_i for i < k (and b = <a', s> + e + m g_level for
 * i = k, as ever).  The expansion is then a GGSW of the reference's form, bit for bit what tfhe_ggsw_encrypt_batch makes
 * from masks a' - m g_level e_i.  The encryption side needs no entry of its own for it: fill the masks, take m g_level off
 * coefficient 0 of mask polynomial i, call tfhe_ggsw_encrypt_batch or the key generation, compress (the Python helpers
 * do).  Rows of LWE and GLWE ciphertexts and of the key-switching key carry their message in the body and need nothing.
 *
 * SECURITY RULE.  One (key, domain, stream) must never produce the masks of two objects encrypted under the same secret
 * key: with equal masks the difference of their bodies is the difference of their messages and errors, in the clear.
 * Draw a fresh 256-bit key per object (the Python helpers do, from the operating system's generator), or number the
 * objects of one client key with `stream`; row ranges of ONE object share its seed and are told apart by first_row.
 *
 * Entry points.  The seed is a HOST struct in both forms and reaches the kernel by value: a captured _device expansion
 * replays its seed (and first_row); only the bodies and the output are read through their pointers at replay.
 * bodies == NULL: the body words of the output are left as they are -- the mask fill of the encryption side (put the
 * errors in the bodies, fill the masks, call the encrypt / keygen entry, compress).
 * Refused with TFHE_ERR_INVALID_ARGUMENT, nothing enqueued and nothing written: a NULL seed or output (compress: input
 * or output); rows == 0 or dimension == 0 (or a dimension of 2^31 or more); a word range that reaches past
 * TFHE_SEED_MAX_WORDS ((first_row + rows) d > 2^36); any overlap of `bodies` and the output; any overlap of input and
 * output in compress.  BMMP, multi-bit, packing and switch keys need no entry of their own: expand on the device, then
 * call the existing _device loader or prepare. */
typedef struct tfhe_seed {
    uint32_t key[8];
    uint64_t stream;
} tfhe_seed;
#define TFHE_SEED_DOMAIN_LWE 0x3145574cu  /* "LWE1" */
#define TFHE_SEED_DOMAIN_GLWE 0x31574c47u /* "GLW1" */
#define TFHE_SEED_MAX_WORDS (1ull << 36)
/* out[i] = G(seed, domain)[first_word + i] for i < count; TFHE_ERR_INVALID_ARGUMENT: NULL seed or out (count != 0), or
 * first_word + count > TFHE_SEED_MAX_WORDS */
int tfhe_seed_words(const tfhe_seed *seed, uint32_t domain, uint64_t first_word, size_t count, uint32_t *out);
/* lwe_out [rows][dimension+1]: masks from the seed, bodies [rows] into the last word of each row (or left, NULL) */
int tfhe_expand_lwe_rows(tfhe_context *ctx, const tfhe_seed *seed, const uint32_t *bodies, uint64_t first_row, size_t rows,
                         size_t dimension, uint32_t *lwe_out);
int tfhe_expand_lwe_rows_device(tfhe_context *ctx, const tfhe_seed *seed, const uint32_t *bodies, uint64_t first_row,
                                size_t rows, size_t dimension, uint32_t *lwe_out);
/* glwe_out [rows][k+1][N]: the k mask polynomials from the seed, bodies [rows][N] into the last (or left, NULL) */
int tfhe_expand_glwe_rows(tfhe_context *ctx, const tfhe_seed *seed, const uint32_t *bodies, uint64_t first_row, size_t rows,
                          uint32_t *glwe_out);
int tfhe_expand_glwe_rows_device(tfhe_context *ctx, const tfhe_seed *seed, const uint32_t *bodies, uint64_t first_row,
                                 size_t rows, uint32_t *glwe_out);
/* the strided gathers of the bodies: bodies_out [rows] of lwe [rows][dimension+1], bodies_out [rows][N] of glwe
 * [rows][k+1][N] */
int tfhe_compress_lwe_rows(tfhe_context *ctx, const uint32_t *lwe, size_t rows, size_t dimension, uint32_t *bodies_out);
int tfhe_compress_lwe_rows_device(tfhe_context *ctx, const uint32_t *lwe, size_t rows, size_t dimension,
                                  uint32_t *bodies_out);
int tfhe_compress_glwe_rows(tfhe_context *ctx, const uint32_t *glwe, size_t rows, uint32_t *bodies_out);
int tfhe_compress_glwe_rows_device(tfhe_context *ctx, const uint32_t *glwe, size_t rows, uint32_t *bodies_out);
/* Host forms only.  tfhe_load_bootstrapping_key from the seeded key: bsk_bodies [n][(k+1)l][N] are GLWE rows 0 ..
 * n (k+1) l - 1 of bsk_seed, ksk_bodies [kN*l_ks] are LWE rows of dimension n of ksk_seed.  The bodies are uploaded, the
 * arrays expanded into a temporary device buffer and handed to tfhe_load_bootstrapping_key_device: the prepared key is
 * byte-identical to the one tfhe_load_bootstrapping_key builds from the expanded arrays. */
int tfhe_load_bootstrapping_key_seeded(tfhe_context *ctx, const tfhe_seed *bsk_seed, const uint32_t *bsk_bodies,
                                       const tfhe_seed *ksk_seed, const uint32_t *ksk_bodies);
/* tfhe_bootstrap_batch on seeded inputs: bodies [batch] are LWE rows first_row .. first_row + batch - 1 of `seed` at the
 * context's boundary dimension (n, or k N with the key switch first); batch words go up instead of batch (dimension + 1) */
int tfhe_bootstrap_batch_seeded(tfhe_context *ctx, const tfhe_seed *seed, uint64_t first_row, const uint32_t *bodies,
                                size_t batch, const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);

/* ---- bootstrap order --------------------------------------------------------------
 * 0 (default): the reference's order, PBS then key switch (bootstrapping.rs:58-120): ciphertexts at
 * the boundary have n+1 words.
 * 1: key switch first (notes/TFHE.md:367-400): input [batch][k*N+1] -> key_switch_lwe -> blind
 * rotation -> sample_extract -> output [batch][k*N+1]; linear combinations between bootstraps then
 * amplify only the PBS noise, not PBS + key-switch noise.  tfhe_bootstrap_batch*, tfhe_gate_batch*,
 * tfhe_lut_gate_batch* and tfhe_lwe_not_batch* all use the selected boundary dimension; the same
 * keys serve both orders. */
int tfhe_context_set_bootstrap_order(tfhe_context *ctx, int ks_first);

/* ---- kernel shape of the blind rotation -----------------------------------------------------------
 * The reference's call shape is ONE ciphertext per bootstrap() (bootstrapping.rs:58-65) and one pair per gate
 * (boolean.rs:9-37).  Two kernels compute the same bits:
 *   TFHE_SHAPE_TEAM  k+1 wave groups per sample (two samples per team where they fit): the throughput shape, the only
 *                    one for the prime-field backends and N = 2048;
 *   TFHE_SHAPE_WIDE  2 (k+1) waves per sample, split by digit level and key part: about half the time per CMUX of one
 *                    sample on an idle chip -- the latency shape (FP64_FFT backend, N <= 1024; elsewhere the team runs);
 *   TFHE_SHAPE_AUTO  (default) the launcher picks by batch: wide while the batch leaves most CUs idle.
 * Affects every entry point that rotates (bootstrap, blind_rotate, gates). */
#define TFHE_SHAPE_AUTO 0
#define TFHE_SHAPE_WIDE 1
#define TFHE_SHAPE_TEAM 2
int tfhe_context_set_kernel_shape(tfhe_context *ctx, int shape);

/* ---- path of the key switch -------------------------------------------------------------------------
 * key_switch_lwe (key_switching.rs:63-103) is out = (0, b) - sum_{i, l} digit_l(a_i) * ksk[i*l_ks + l], a wrapping-u32
 * matrix product of small digits with a key that is constant between loads.  Two kernels compute the same bits:
 *   TFHE_KS_PATH_SCALAR  one 32-bit multiply-add per term on the vector units: every parameter set;
 *   TFHE_KS_PATH_MATRIX  the key as four signed byte planes (prepared at key load, 4 k N l_ks (n+1) more bytes plus
 *                        padding to whole tiles), exact int8 x int8 -> int32 products on the matrix cores, the planes
 *                        folded as sum_j plane_j << 8j.  Needs digits that fit int8 -- key-switch log_base <= 6: the
 *                        literal decomposer can emit the value B itself -- and k N l_ks 2^(log_base + 7) < 2^31, so that
 *                        no plane sum overflows; TFHE_ERR_UNSUPPORTED otherwise;
 *   TFHE_KS_PATH_AUTO    (default) the matrix path wherever it is admitted (it measured faster at every batch, 1 to
 *                        4,096), the scalar kernel elsewhere.
 * Affects every entry point that key-switches (bootstrap in both orders, gates, tree LUTs, tfhe_key_switch_batch*). */
#define TFHE_KS_PATH_AUTO 0
#define TFHE_KS_PATH_SCALAR 1
#define TFHE_KS_PATH_MATRIX 2
int tfhe_context_set_key_switch_path(tfhe_context *ctx, int path);
/* How a key switch of `batch` ciphertexts would go out under the current path: *path = TFHE_KS_PATH_SCALAR or
 * TFHE_KS_PATH_MATRIX, the grid of workgroups (column tiles x sample tiles) and the shares of the mask words (more than
 * one: the output is zeroed first and partial sums are added). */
int tfhe_debug_key_switch_plan(tfhe_context *ctx, size_t batch, int *path, unsigned *grid_x, unsigned *grid_y,
                               unsigned *splits);

/* ---- decomposer alignment ------------------------------------------------------
 * 0 (default): the reference's literal decomposer -- limbs counted from bit 0 (decomposer.rs:48-70),
 * gadget factors beta^{floor(32/log_base)-(level+1)} (ggsw.rs:98, key_switching.rs:38), bit-exact
 * with the crate; when log_base does not divide 32 the top 32 mod log_base bits are never
 * represented, so such parameter sets do not decrypt (the reference's notes leave beta^l != q as a
 * TODO, notes/TFHE.md:116,407).
 * 1: aligned -- limbs and gadget factors counted down from bit 32 (factor 2^{32-log_base*(level+1)}),
 * which makes e.g. log_base = 7, levels = 3 a working parameter set.  Applies to both decomposers,
 * to the hot path and to keygen; identical bits to mode 0 whenever log_base divides 32.  Keys made
 * in one mode must be used in that mode. */
int tfhe_context_set_decomposer_alignment(tfhe_context *ctx, int aligned);

/* ---- on-disk format for keys and ciphertexts (the reference has none) -----------
 * One array per file, host side only (no GPU needed), little endian:
 *   0   char[8]  magic "TFHEAMD\1"
 *   8   u32      kind (TFHE_FILE_*)          12  u32  flags (bit 0: aligned decomposer)
 *   16  u32[12]  tfhe_params (k, log2 N, n, padding_bits, log_p, log_q, ks{log_base, levels, log_q},
 *                pbs{log_base, levels, log_q})
 *   64  u32      ndims (1..4)                68  u32[4] dims (row-major, unused = 1)   84  u32  0
 *   88  u64      payload words (= product of dims)
 *   96  u64      FNV-1a 64 of the payload bytes
 *   104 u32[]    payload: the array exactly as the ABI takes it (reference layouts)
 * Readers refuse a wrong magic, a size that disagrees with the header, and a checksum mismatch
 * (TFHE_ERR_IO); comparing the stored parameters with the context's is the caller's job
 * (tfhe_file_read_header hands them back). */
#define TFHE_FILE_BSK 1   /* [n][(k+1)l][k+1][N] */
#define TFHE_FILE_KSK 2   /* [kN*l_ks][n+1] */
#define TFHE_FILE_LWE 3   /* [batch][dim+1] */
#define TFHE_FILE_GLWE 4  /* [batch][k+1][N] */
#define TFHE_FILE_GGSW 5  /* [count][(k+1)l][k+1][N] */
#define TFHE_FILE_WORDS 6 /* any other u32 array (test vectors [N], mod-switched masks, ...) */
#define TFHE_FILE_PKSK 7  /* [from_dimension*l_ks][k+1][N] (tfhe_generate_packing_key) */
#define TFHE_FILE_FLAG_ALIGNED 1u
int tfhe_file_write(const char *path, uint32_t kind, const tfhe_params *params, uint32_t flags,
                    const uint32_t *dims, uint32_t ndims, const uint32_t *data);
int tfhe_file_read_header(const char *path, uint32_t *kind, tfhe_params *params, uint32_t *flags,
                          uint32_t dims[4], uint32_t *ndims, uint64_t *words);
int tfhe_file_read(const char *path, uint32_t *data, uint64_t words);

/* ---- multi-GPU pool ----------------------------------------------------------------
 * The reference's shape is ONE BootstrappingKey (bootstrapping.rs:18-21) and many independent bootstrap() calls
 * (bootstrapping.rs:58-65; the gates of boolean.rs:9-53 are one bootstrap each).  A pool holds one context per listed
 * HIP device: the key is uploaded and transformed ONCE (member 0) and the PREPARED key is replicated device to device
 * (peer copies over xGMI, concurrently on the destination members' streams -- not N host uploads and N prepares); a
 * batch is cut into contiguous slices, slice i = [i*q + min(i, r), ...) of q = batch / n (+1 for the first r =
 * batch % n members), and there is no collective anywhere in the data path.  Same bits as a single context: every
 * bootstrap is a pure function of (ciphertext, test vector, keys).
 * A device may be listed more than once (several members on one GPU); that is how a one-GPU box tests the pool.
 * Host-pointer calls block until the results are in host memory and run one host thread per member; a pool must not
 * be used from two threads at once. */
typedef struct tfhe_pool tfhe_pool;
int tfhe_pool_create(const tfhe_params *params, const int *devices, size_t n_devices, int backend,
                     tfhe_pool **out);
void tfhe_pool_destroy(tfhe_pool *pool);
size_t tfhe_pool_size(const tfhe_pool *pool);
/* Borrowed handle of member i (owned by the pool): for the per-context introspection calls (timing, backend name). */
tfhe_context *tfhe_pool_member(tfhe_pool *pool, size_t i);
const char *tfhe_pool_last_error(const tfhe_pool *pool);
/* The slice of a batch member `member` processes: rows [*first, *first + *count). */
int tfhe_pool_shard(const tfhe_pool *pool, size_t batch, size_t member, size_t *first, size_t *count);
/* tfhe_context_set_decomposer_alignment / _set_bootstrap_order / _reserve / _synchronize for every member
 * (reserve sizes each member for its slice of `max_batch`). */
int tfhe_pool_set_decomposer_alignment(tfhe_pool *pool, int aligned);
int tfhe_pool_set_bootstrap_order(tfhe_pool *pool, int ks_first);
int tfhe_pool_set_kernel_shape(tfhe_pool *pool, int shape); /* tfhe_context_set_kernel_shape for every member */
int tfhe_pool_set_key_switch_path(tfhe_pool *pool, int path); /* tfhe_context_set_key_switch_path for every member */
/* tfhe_debug_key_switch_plan of member `member` for its slice of `batch` */
int tfhe_pool_debug_key_switch_plan(tfhe_pool *pool, size_t member, size_t batch, int *path, unsigned *grid_x,
                                    unsigned *grid_y, unsigned *splits);
int tfhe_pool_reserve(tfhe_pool *pool, size_t max_batch);
int tfhe_pool_synchronize(tfhe_pool *pool);
/* BootstrappingKey upload, layouts as tfhe_load_bootstrapping_key: host pointers, or (_device) pointers on member
 * 0's device. */
int tfhe_pool_load_bootstrapping_key(tfhe_pool *pool, const uint32_t *bsk, const uint32_t *ksk);
int tfhe_pool_load_bootstrapping_key_device(tfhe_pool *pool, const uint32_t *bsk, const uint32_t *ksk);
/* the BMMP key of tfhe_load_bootstrapping_key_bmmp, replicated the same way */
int tfhe_pool_load_bootstrapping_key_bmmp(tfhe_pool *pool, const uint32_t *bsk_bmmp, const uint32_t *ksk);
/* bootstrapping_key_gen (bootstrapping.rs:23-56) on the pool: arguments as tfhe_bootstrapping_key_gen[_bmmp], the key is
 * generated on member 0's device and, with `load` != 0, installed on EVERY member (prepared once, replicated device to
 * device like an uploaded key).  tfhe_pool_replicate_key re-replicates whatever key member 0 holds -- after a call that
 * installed a key on tfhe_pool_member(pool, 0) alone, e.g. tfhe_bootstrapping_key_gen_device with load. */
int tfhe_pool_bootstrapping_key_gen(tfhe_pool *pool, const uint32_t *lwe_sk, const uint32_t *glwe_sk,
                                    uint32_t *bsk, uint32_t *ksk, int load);
int tfhe_pool_bootstrapping_key_gen_bmmp(tfhe_pool *pool, const uint32_t *lwe_sk, const uint32_t *glwe_sk,
                                         uint32_t *bsk_bmmp, uint32_t *ksk, int load);
int tfhe_pool_replicate_key(tfhe_pool *pool);
/* bootstrap() over a host batch sharded across the members; arguments as tfhe_bootstrap_batch. */
int tfhe_pool_bootstrap_batch(tfhe_pool *pool, const uint32_t *lwe_in, size_t batch,
                              const uint32_t *test_vector_poly, size_t tv_count, uint32_t *lwe_out);
/* and()/or()/... over a host batch sharded across the members; arguments as tfhe_gate_batch. */
int tfhe_pool_gate_batch(tfhe_pool *pool, const uint32_t truth[4], const uint32_t *ct0,
                         const uint32_t *ct1, size_t batch, uint32_t *lwe_out);
/* Device-resident shards: member i bootstraps counts[i] ciphertexts at lwe_in[i] (a pointer on ITS device) with
 * test vector(s) tv[i] (tv_counts[i] = 1 or counts[i]) into lwe_out[i].  Enqueues on every member's stream and
 * returns; tfhe_pool_synchronize waits.  counts[i] = 0 skips a member.  Arguments of all members are checked before
 * anything is enqueued (a failing call has launched nothing).
 * ORDERING CONTRACT: member i's work runs on member i's stream -- its own non-blocking stream unless
 * tfhe_context_set_stream(tfhe_pool_member(pool, i), s) gave it one.  The call does NOT order against whatever stream
 * produced lwe_in[i] / tv[i] or will consume lwe_out[i]: the caller synchronises those producers first (or hands every
 * member the producing stream), and must keep the buffers alive until tfhe_pool_synchronize. */
int tfhe_pool_bootstrap_shards_device(tfhe_pool *pool, const uint32_t *const *lwe_in, const size_t *counts,
                                      const uint32_t *const *test_vector_poly, const size_t *tv_counts,
                                      uint32_t *const *lwe_out);

/* ---- introspection for benchmarks --------------------------------------------------------- */
/* Time of the blind-rotation kernel of the most recent bootstrap/blind_rotate call, measured with
 * HIP events on the context's stream (milliseconds); negative if none was recorded.  Enable with
 * tfhe_context_set_timing(ctx, 1): the _device calls then record events (still no sync). */
int tfhe_context_set_timing(tfhe_context *ctx, int enable);
int tfhe_last_kernel_ms(tfhe_context *ctx, float *blind_rotate_ms, float *key_switch_ms);
/* The same for the bootstrap (or gate) call made `steps_ago` timed calls before the last one (0 = the last; the
 * context keeps the events of the last 64): K steps can be enqueued back to back and read afterwards, with no host
 * synchronisation inside the timed loop. */
int tfhe_kernel_ms_ago(tfhe_context *ctx, unsigned steps_ago, float *blind_rotate_ms, float *key_switch_ms);
/* HBM roofline measured on this device now: a 16-byte-per-lane stream copy of `bytes` (two scratch
 * buffers are allocated and freed inside), `reps` timed launches on the context's stream;
 * *gb_per_s = (bytes read + bytes written) / time.  Synchronises. */
int tfhe_measure_hbm_copy(tfhe_context *ctx, size_t bytes, int reps, double *gb_per_s);

/* Rounding-margin probe of the FP64_FFT backend (test instrumentation, not a reference function): the largest
 * |value - nearest integer| any lane has lifted on the device since the last reset -- the measured counterpart of
 * the proven bound in csrc/field_fft.h.  Only the probe build (libtfhe_hip_probe.so, -DTFHE_FFT_TRACK_ERROR; kept
 * beside the product library, never loaded by it) records it; the product library returns TFHE_ERR_UNSUPPORTED.
 * Synchronises the device. */
int tfhe_debug_fft_margin(tfhe_context *ctx, double *worst, int reset);

/* How tfhe_bootstrap_batch[_device] sends out the blind rotations of a batch of this size (no reference counterpart;
 * bench lines and tests).  A batch larger than what the chip rotates at once (*resident_samples) goes out in groups of
 * *samples_per_group samples; every rotation is cut into *segments launches that walk a slice of the bootstrapping key each
 * (the accumulators wait in the context's workspace in between: tfhe_context_reserve), and with *streams == 2 the two
 * halves of a group alternate on the context's stream and a second stream of its own, which is joined before the call
 * returns -- the caller still orders everything on the one stream it gave (tfhe_context_set_stream). */
int tfhe_debug_blind_rotate_plan(tfhe_context *ctx, size_t batch, size_t *samples_per_group, unsigned *segments,
                                 unsigned *streams, size_t *resident_samples);

/* The kernel shape behind that plan: waves of one workgroup that work on a sample's rotation -- (k+1) x waves per
 * polynomial for the throughput kernel (shared by *samples_per_team samples where two fit), 2 (k+1) for the wide team
 * that batches too small to fill the chip get (one sample per workgroup; the latency shape of the reference's
 * one-ciphertext bootstrap(), bootstrapping.rs:58-65). */
int tfhe_debug_blind_rotate_shape(tfhe_context *ctx, size_t batch, unsigned *waves_per_sample,
                                  unsigned *samples_per_team);

/* Library / build identification */
const char *tfhe_version(void);

#ifdef __cplusplus
}
#endif
#endif
