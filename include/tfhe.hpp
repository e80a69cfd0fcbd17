// tfhe.hpp -- C++17 host-side mirror of the reference crate's bootstrapping-path interface, over
// the C ABI of include/tfhe_hip.h.
//
// The reference (Janmajayamall/tfhe-research) is Rust; this image has no Rust toolchain, so the
// host side above the C ABI is written in C++ with the reference's names, argument meaning and
// error behaviour (its panics become C++ exceptions thrown HERE, never across the C ABI), so that
// tests read like the reference's own.  A Rust shim with the same shape is shipped as source in
// rust/ and described in INTEGRATION.md.  Citations are file:line under /root/reference/src.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <cmath>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "tfhe_hip.h"

namespace tfhe_amd {

struct TfheError : std::runtime_error {
  int status;
  TfheError(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};

// decomposer.rs:2-16
struct DecomposerParams {
  uint32_t log_base, levels, log_q;
  DecomposerParams(uint32_t log_base_, uint32_t levels_, uint32_t log_q_ = 32)
      : log_base(log_base_), levels(levels_), log_q(log_q_) {}
};

// lib.rs:23-74.  Fields are public here (the reference's are private with no constructor, which
// makes every non-default parameter set unconstructible from outside the crate).
struct TfheParams {
  uint32_t glwe_dimension = 2;
  uint32_t glwe_poly_degree = 9;  // log2 N (lib.rs:40)
  uint32_t lwe_dimension = 722;
  uint32_t padding_bits = 1;
  uint32_t log_p = 2;
  uint32_t log_q = 32;
  DecomposerParams ks_decomposer{4, 5, 32};
  DecomposerParams pbs_decomposer{4, 6, 32};
  double lwe_std_dev = 0.000013071021089943935;    // lib.rs:96,120
  double glwe_std_dev = 0.00000004990272175010415;  // lib.rs:97,121

  static TfheParams default_params() { return TfheParams{}; }  // lib.rs:101-123
  static TfheParams default_test_params() {                    // lib.rs:77-99
    TfheParams p;
    p.lwe_dimension = 4;
    return p;
  }
  size_t degree() const { return size_t(1) << glwe_poly_degree; }             // glwe.rs:124-127
  size_t lwe_dimension_post_pbs() const { return degree() * glwe_dimension; }  // lib.rs:58-66
  size_t ggsw_rows() const { return size_t(glwe_dimension + 1) * pbs_decomposer.levels; }

  tfhe_params c() const {
    tfhe_params p;
    p.glwe_dimension = glwe_dimension;
    p.glwe_poly_degree = glwe_poly_degree;
    p.lwe_dimension = lwe_dimension;
    p.padding_bits = padding_bits;
    p.log_p = log_p;
    p.log_q = log_q;
    p.ks_decomposer = {ks_decomposer.log_base, ks_decomposer.levels, ks_decomposer.log_q};
    p.pbs_decomposer = {pbs_decomposer.log_base, pbs_decomposer.levels, pbs_decomposer.log_q};
    return p;
  }
};

// lwe.rs:110-115: data = (a_0, ..., a_{n-1}, b)
struct LweCiphertext {
  std::vector<uint32_t> data;
};
// lwe.rs:9-15
inline LweCiphertext operator+(const LweCiphertext& a, const LweCiphertext& b) {
  if (a.data.size() != b.data.size()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length mismatch");
  LweCiphertext r{a.data};
  for (size_t i = 0; i < r.data.size(); ++i) r.data[i] += b.data[i];
  return r;
}
// lwe.rs:17-23
inline LweCiphertext operator*(const LweCiphertext& a, uint32_t rhs) {
  LweCiphertext r{a.data};
  for (auto& v : r.data) v *= rhs;
  return r;
}

// glwe.rs:185-188: row-major (k+1, N), body last
struct GlweCiphertext {
  std::vector<uint32_t> data;
};
// ggsw.rs:37-41: ((k+1)*l, k+1, N), row = poly_index*l + level
struct GgswCiphertext {
  std::vector<uint32_t> data;
};
// key_switching.rs:13-15: (k*N*l_ks, n+1)
struct KeySwitchingKey {
  std::vector<uint32_t> data;
};
// bootstrapping.rs:18-21
struct BootstrappingKey {
  std::vector<GgswCiphertext> lwe_sk_ggsw_enc;
  KeySwitchingKey ksk;
};
// glwe.rs:16-18
struct Monomial {
  int64_t index;
};

// The GPU engine: owns the device-side (NTT-domain) copies of ONE BootstrappingKey on one or several GPUs.
// With a device list it is a pool (tfhe_pool_*, tfhe_hip.h): the key is uploaded and transformed once and the
// prepared key replicated device to device; bootstrap_batch() and gate_batch() cut their batch into contiguous
// slices, one per device; the single-ciphertext functions run on the first device.  Same bits either way.
class Engine {
 public:
  // backend: TFHE_BACKEND_AUTO, or one of the transforms of tfhe_hip.h (every one returns the same bits;
  // TFHE_ERR_EXACTNESS / TFHE_ERR_UNSUPPORTED if the parameter set is outside the chosen one's bound or shapes)
  explicit Engine(const TfheParams& params, int device = 0, int backend = TFHE_BACKEND_AUTO)
      : Engine(params, std::vector<int>{device}, backend) {}
  // one member per entry of `devices` (HIP device ordinals; an ordinal may repeat)
  Engine(const TfheParams& params, const std::vector<int>& devices, int backend = TFHE_BACKEND_AUTO) : params_(params) {
    tfhe_params cp = params.c();
    tfhe_pool* raw = nullptr;
    int st = tfhe_pool_create(&cp, devices.data(), devices.size(), backend, &raw);
    if (st != TFHE_OK) throw TfheError(st, std::string("tfhe_pool_create: ") + tfhe_status_string(st));
    pool_.reset(raw);
    ctx_ = tfhe_pool_member(raw, 0);
  }
  // "fp64-fft", "fp64-p49", "fp64-p42", "goldilocks" or "goldilocks-split"
  std::string backend() const { return tfhe_context_backend(ctx_); }
  size_t devices() const { return tfhe_pool_size(pool_.get()); }

  // Uploads the key in the reference's own layout (n separate GGSW arrays + the KSK array).  A key of
  // the unrolled blind rotation (notes/BMMP Bootstrapping.md; bootstrapping_key_gen_bmmp below) holds
  // 3 GGSWs per pair of key bits instead: pass bmmp = true; bootstrap() and the gates then use it.
  void load(const BootstrappingKey& bk, bool bmmp = false) {
    const size_t ggsw_words = params_.ggsw_rows() * (params_.glwe_dimension + 1) * params_.degree();
    if (bk.lwe_sk_ggsw_enc.size() != (bmmp ? params_.lwe_dimension / 2 * 3 : params_.lwe_dimension))
      throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "bootstrapping key must hold n (BMMP: 3n/2) GGSW ciphertexts");
    std::vector<uint32_t> flat;
    flat.reserve(ggsw_words * bk.lwe_sk_ggsw_enc.size());
    for (const auto& g : bk.lwe_sk_ggsw_enc) {
      if (g.data.size() != ggsw_words) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GGSW shape");
      flat.insert(flat.end(), g.data.begin(), g.data.end());
    }
    const size_t ksk_words = params_.lwe_dimension_post_pbs() * params_.ks_decomposer.levels *
                             (size_t(params_.lwe_dimension) + 1);
    if (bk.ksk.data.size() != ksk_words) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "KSK shape");
    check_pool(bmmp ? tfhe_pool_load_bootstrapping_key_bmmp(pool_.get(), flat.data(), bk.ksk.data.data())
                    : tfhe_pool_load_bootstrapping_key(pool_.get(), flat.data(), bk.ksk.data.data()));
  }
  bool uses_bmmp() const { return tfhe_context_uses_bmmp(ctx_) != 0; }

  // Extensions beyond the reference (tfhe_hip.h): the aligned decomposer for bases with
  // beta^l != q, and the key-switch-then-PBS order of notes/TFHE.md:367-400 (ciphertexts of
  // k*N+1 words at the boundary).  Defaults are the reference's behaviour.
  void set_decomposer_alignment(bool aligned) { check_pool(tfhe_pool_set_decomposer_alignment(pool_.get(), aligned)); }
  void set_bootstrap_order(bool ks_first) { check_pool(tfhe_pool_set_bootstrap_order(pool_.get(), ks_first)); }
  // TFHE_SHAPE_AUTO (default: by batch size), TFHE_SHAPE_WIDE (the latency shape: the reference's bootstrap() takes ONE
  // ciphertext, bootstrapping.rs:58-65) or TFHE_SHAPE_TEAM for every blind rotation of the engine; same bits either way
  void set_kernel_shape(int shape) { check_pool(tfhe_pool_set_kernel_shape(pool_.get(), shape)); }
  // TFHE_KS_PATH_AUTO (default), TFHE_KS_PATH_SCALAR or TFHE_KS_PATH_MATRIX (int8 matrix cores over the prepared key;
  // throws where the key-switch digits do not fit int8) for every key_switch_lwe (key_switching.rs:63-103); same bits
  void set_key_switch_path(int path) { check_pool(tfhe_pool_set_key_switch_path(pool_.get(), path)); }

  const TfheParams& params() const { return params_; }
  tfhe_context* raw() const { return ctx_; }        // the first device's context (single-ciphertext calls)
  tfhe_pool* raw_pool() const { return pool_.get(); }  // all devices (batch calls)
  void check(int st) const {
    if (st != TFHE_OK) throw TfheError(st, std::string(tfhe_status_string(st)) + ": " + tfhe_last_error(ctx_));
  }
  void check_pool(int st) const {
    if (st != TFHE_OK) throw TfheError(st, std::string(tfhe_status_string(st)) + ": " + tfhe_pool_last_error(pool_.get()));
  }

 private:
  struct Deleter {
    void operator()(tfhe_pool* p) const { tfhe_pool_destroy(p); }
  };
  TfheParams params_;
  std::unique_ptr<tfhe_pool, Deleter> pool_;
  tfhe_context* ctx_ = nullptr;  // member 0, owned by the pool
};

// test_vector.rs:38-67
inline std::vector<uint32_t> construct_test_from_lut(const TfheParams& p, const std::vector<uint32_t>& lut) {
  std::vector<uint32_t> out(p.degree());
  tfhe_params cp = p.c();
  int st = tfhe_construct_test_from_lut(&cp, lut.data(), lut.size(), out.data());
  if (st != TFHE_OK) throw TfheError(st, "construct_test_from_lut: lut must hold 2^log_p entries (test_vector.rs:41)");
  return out;
}
// test_vector.rs:23-35
inline std::vector<uint32_t> construct_identity_test_vector(const TfheParams& p) {
  std::vector<uint32_t> lut(size_t(1) << p.log_p);
  for (size_t i = 0; i < lut.size(); ++i) lut[i] = uint32_t(i);
  return construct_test_from_lut(p, lut);
}
// test_vector.rs:5-20: f(lhs, rhs)
inline std::vector<uint32_t> construct_test_vector_boolean(const TfheParams& p,
                                                           const std::function<uint32_t(uint32_t, uint32_t)>& f) {
  std::vector<uint32_t> lut(size_t(1) << p.log_p);
  for (size_t i = 0; i < lut.size(); ++i) lut[i] = f(uint32_t(i >> 1) & 1u, uint32_t(i) & 1u);
  return construct_test_from_lut(p, lut);
}

// bootstrap(): bootstrapping.rs:58-120, over a batch that shares one test vector.  The engine
// replaces the reference's `&BootstrappingKey` argument (the key lives on the GPU after load()).
inline std::vector<LweCiphertext> bootstrap_batch(Engine& e, const std::vector<LweCiphertext>& cts,
                                                  const std::vector<uint32_t>& test_vector_poly) {
  const size_t n1 = size_t(e.params().lwe_dimension) + 1;
  std::vector<uint32_t> in(cts.size() * n1), out(cts.size() * n1);
  for (size_t b = 0; b < cts.size(); ++b) {
    if (cts[b].data.size() != n1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
    std::copy(cts[b].data.begin(), cts[b].data.end(), in.begin() + b * n1);
  }
  // sharded over the engine's devices (one device: the plain single-context path)
  e.check_pool(tfhe_pool_bootstrap_batch(e.raw_pool(), in.data(), cts.size(), test_vector_poly.data(), 1, out.data()));
  std::vector<LweCiphertext> res(cts.size());
  for (size_t b = 0; b < cts.size(); ++b) res[b].data.assign(out.begin() + b * n1, out.begin() + (b + 1) * n1);
  return res;
}
inline LweCiphertext bootstrap(Engine& e, const LweCiphertext& lwe_ciphertext,
                               const std::vector<uint32_t>& test_vector_poly) {
  return bootstrap_batch(e, {lwe_ciphertext}, test_vector_poly)[0];
}

// key_switch_lwe(): key_switching.rs:63-103 (from the post-PBS dimension to n, with the loaded KSK)
inline LweCiphertext key_switch_lwe(Engine& e, const LweCiphertext& ct) {
  LweCiphertext out{std::vector<uint32_t>(size_t(e.params().lwe_dimension) + 1)};
  if (ct.data.size() != e.params().lwe_dimension_post_pbs() + 1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
  e.check(tfhe_key_switch_batch(e.raw(), ct.data.data(), 1, out.data.data()));
  return out;
}

// external_product(): ggsw.rs:132-161
inline GlweCiphertext external_product(Engine& e, const GgswCiphertext& ggsw, const GlweCiphertext& glwe) {
  GlweCiphertext out{std::vector<uint32_t>(glwe.data.size())};
  e.check(tfhe_external_product_batch(e.raw(), ggsw.data.data(), 1, glwe.data.data(), 1, out.data.data()));
  return out;
}
// cmux(): ggsw.rs:164-178 -- mutates glwe_ciphertext1 (ct1 -= ct0) like the reference
inline GlweCiphertext cmux(Engine& e, const GgswCiphertext& ggsw, const GlweCiphertext& glwe_ciphertext0,
                           GlweCiphertext& glwe_ciphertext1) {
  GlweCiphertext out{std::vector<uint32_t>(glwe_ciphertext0.data.size())};
  e.check(tfhe_cmux_batch(e.raw(), ggsw.data.data(), 1, glwe_ciphertext0.data.data(),
                          glwe_ciphertext1.data.data(), 1, out.data.data()));
  return out;
}
// &GlweCiphertext * &Monomial: glwe.rs:20-34
inline GlweCiphertext operator_mul(Engine& e, const GlweCiphertext& glwe, const Monomial& m) {
  GlweCiphertext out{std::vector<uint32_t>(glwe.data.size())};
  e.check(tfhe_glwe_mul_monomial_batch(e.raw(), glwe.data.data(), 1, &m.index, out.data.data()));
  return out;
}
// sample_extract(): bootstrapping.rs:122-156
inline LweCiphertext sample_extract(Engine& e, const GlweCiphertext& glwe, size_t sample_index) {
  LweCiphertext out{std::vector<uint32_t>(e.params().lwe_dimension_post_pbs() + 1)};
  e.check(tfhe_sample_extract_batch(e.raw(), glwe.data.data(), 1, sample_index, out.data.data()));
  return out;
}

// SignedDecomposer: decomposer.rs:18-96 (decompose runs on the device; round/recompose are trivial)
class SignedDecomposer {
 public:
  SignedDecomposer(Engine& e, int which) : e_(e), which_(which) {}
  std::vector<uint32_t> decompose(uint32_t value) const {  // decomposer.rs:42-80
    const auto& d = which_ == TFHE_DECOMPOSER_PBS ? e_.params().pbs_decomposer : e_.params().ks_decomposer;
    std::vector<uint32_t> out(d.levels);
    e_.check(tfhe_decompose(e_.raw(), which_, &value, 1, out.data()));
    return out;
  }

 private:
  Engine& e_;
  int which_;
};

// and()/or(): boolean.rs:9-53, plus the gates the reference leaves to the closure hook
inline LweCiphertext gate(Engine& e, const uint32_t truth[4], const LweCiphertext& ct0, const LweCiphertext& ct1) {
  LweCiphertext out{std::vector<uint32_t>(ct0.data.size())};
  e.check(tfhe_gate_batch(e.raw(), truth, ct0.data.data(), ct1.data.data(), 1, out.data.data()));
  return out;
}
// a stream of gates with one truth table, sharded over the engine's devices (boolean.rs:9-53 per pair)
inline std::vector<LweCiphertext> gate_batch(Engine& e, const uint32_t truth[4], const std::vector<LweCiphertext>& ct0,
                                             const std::vector<LweCiphertext>& ct1) {
  if (ct0.size() != ct1.size() || ct0.empty()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "gate_batch: equal, non-zero counts");
  const size_t w = ct0[0].data.size();
  std::vector<uint32_t> a(ct0.size() * w), b(ct0.size() * w), out(ct0.size() * w);
  for (size_t i = 0; i < ct0.size(); ++i) {
    if (ct0[i].data.size() != w || ct1[i].data.size() != w) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
    std::copy(ct0[i].data.begin(), ct0[i].data.end(), a.begin() + i * w);
    std::copy(ct1[i].data.begin(), ct1[i].data.end(), b.begin() + i * w);
  }
  e.check_pool(tfhe_pool_gate_batch(e.raw_pool(), truth, a.data(), b.data(), ct0.size(), out.data()));
  std::vector<LweCiphertext> res(ct0.size());
  for (size_t i = 0; i < ct0.size(); ++i) res[i].data.assign(out.begin() + i * w, out.begin() + (i + 1) * w);
  return res;
}
inline LweCiphertext and_(Engine& e, const LweCiphertext& ct0, const LweCiphertext& ct1) {
  const uint32_t t[4] = {0, 0, 0, 1};
  return gate(e, t, ct0, ct1);
}
inline LweCiphertext or_(Engine& e, const LweCiphertext& ct0, const LweCiphertext& ct1) {
  const uint32_t t[4] = {0, 1, 1, 1};
  return gate(e, t, ct0, ct1);
}
inline LweCiphertext nand(Engine& e, const LweCiphertext& ct0, const LweCiphertext& ct1) {
  const uint32_t t[4] = {1, 1, 1, 0};
  return gate(e, t, ct0, ct1);
}
inline LweCiphertext xor_(Engine& e, const LweCiphertext& ct0, const LweCiphertext& ct1) {
  const uint32_t t[4] = {0, 1, 1, 0};
  return gate(e, t, ct0, ct1);
}
// Gates beyond the reference's two, by notes/Boolean Gates.md:2-11.
// NOT needs no bootstrap: (-a, enc(1) - b)
inline LweCiphertext not_(Engine& e, const LweCiphertext& ct) {
  LweCiphertext out{std::vector<uint32_t>(ct.data.size())};
  e.check(tfhe_lwe_not_batch(e.raw(), ct.data.data(), 1, out.data.data()));
  return out;
}
// gate of m inputs: one PBS of sum_i 2^i * cts[i] (cts[0] = rightmost input), truth has 2^m entries;
// needs params.log_p >= m
inline LweCiphertext lut_gate(Engine& e, const std::vector<uint32_t>& truth, const std::vector<const LweCiphertext*>& cts) {
  if (cts.empty() || truth.size() != (size_t(1) << cts.size())) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "truth table size");
  std::vector<const uint32_t*> ptrs;
  for (const LweCiphertext* c : cts) ptrs.push_back(c->data.data());
  LweCiphertext out{std::vector<uint32_t>(cts[0]->data.size())};
  e.check(tfhe_lut_gate_batch(e.raw(), truth.data(), (uint32_t)cts.size(), ptrs.data(), 1, out.data.data()));
  return out;
}
// sel ? a : b with two bootstraps at any log_p >= 2: AND(sel, a) + AND(NOT sel, b)
inline LweCiphertext mux(Engine& e, const LweCiphertext& sel, const LweCiphertext& a, const LweCiphertext& b) {
  const uint32_t t_and[4] = {0, 0, 0, 1}, t_andnot[4] = {0, 1, 0, 0};  // truth[(lhs << 1) | rhs], lhs = sel
  return gate(e, t_and, a, sel) + gate(e, t_andnot, b, sel);
}

// ------------------------------------------------------------------------------------------------
// Encryption side.  The reference threads `rng: &mut R` through keygen and
// encryption; here `Rng` is any C++ UniformRandomBitGenerator.  The draws happen on the host, in
// the reference's order (masks with sample_uniform_array, errors with sample_gaussian_array), and
// land in the output buffer; the GPU then adds the <mask, key> terms and the messages.
// ------------------------------------------------------------------------------------------------
// utils.rs:36-41, but two-sided: the reference's `frac as u32` saturates negative errors to 0
// (a one-sided error distribution); a negative error wraps mod 2^32 here.
inline uint32_t f64_to_torus_unsigned_representation(double v) {
  double frac = v - std::round(v);
  frac = std::round(frac * 4294967296.0);
  return static_cast<uint32_t>(static_cast<uint64_t>(static_cast<int64_t>(frac)));
}
template <class Rng>
void sample_uniform_slice(Rng& rng, uint32_t* out, size_t len) {  // utils.rs:56-66
  std::uniform_int_distribution<uint32_t> d;
  for (size_t i = 0; i < len; ++i) out[i] = d(rng);
}
template <class Rng>
void sample_gaussian_slice(double std_dev, Rng& rng, uint32_t* out, size_t len) {  // utils.rs:43-54
  std::normal_distribution<double> d(0.0, std_dev);
  for (size_t i = 0; i < len; ++i) out[i] = f64_to_torus_unsigned_representation(d(rng));
}
template <class Rng>
void sample_binary_slice(Rng& rng, uint32_t* out, size_t len) {  // utils.rs:68-93
  std::uniform_int_distribution<unsigned> byte(0, 255);
  unsigned cur = byte(rng), bit = 0;
  for (size_t i = 0; i < len; ++i) {
    out[i] = (cur >> bit) & 1u;
    if (++bit == 8) {
      cur = byte(rng);
      bit = 0;
    }
  }
}

// lwe.rs:47-60
struct LweSecretKey {
  std::vector<uint32_t> data;
  template <class Rng>
  static LweSecretKey random(size_t lwe_dimension, Rng& rng) {
    LweSecretKey sk{std::vector<uint32_t>(lwe_dimension)};
    sample_binary_slice(rng, sk.data.data(), sk.data.size());
    return sk;
  }
};
// glwe.rs:171-182: (k, N) row-major
struct GlweSecretKey {
  std::vector<uint32_t> data;
  template <class Rng>
  static GlweSecretKey random(const TfheParams& p, Rng& rng) {
    GlweSecretKey sk{std::vector<uint32_t>(p.glwe_dimension * p.degree())};
    sample_binary_slice(rng, sk.data.data(), sk.data.size());
    return sk;
  }
};
// LweSecretKey::from(&GlweSecretKey) lwe.rs:62-73: the row-major flattening
inline LweSecretKey lwe_secret_key_from(const GlweSecretKey& sk) { return LweSecretKey{sk.data}; }

// LweCleartext::encode_message lwe.rs:81-92 / LwePlaintext::decode lwe.rs:100-107
inline uint32_t encode_message(uint32_t m, const TfheParams& p) {
  if (m >= (1u << p.log_p)) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "assertion failed: m < 1 << log_p");
  return m << (p.log_q - (p.log_p + p.padding_bits));
}
inline uint32_t decode_plaintext(uint32_t pt, const TfheParams& p) {
  return pt >> (p.log_q - (p.log_p + p.padding_bits));
}

// encrypt_lwe_plaintext lwe.rs:138-160 (draw order: error, then mask); `plaintext` is encoded
template <class Rng>
LweCiphertext encrypt_lwe_plaintext(Engine& e, double std_dev, const LweSecretKey& sk, uint32_t plaintext,
                                    Rng& rng) {
  const size_t n = sk.data.size();
  LweCiphertext ct{std::vector<uint32_t>(n + 1)};
  sample_gaussian_slice(std_dev, rng, &ct.data[n], 1);
  sample_uniform_slice(rng, ct.data.data(), n);
  e.check(tfhe_lwe_encrypt_batch(e.raw(), sk.data.data(), n, &plaintext, ct.data.data(), 1));
  return ct;
}
// decrypt_lwe lwe.rs:162-173 -> encoded plaintext
inline uint32_t decrypt_lwe(Engine& e, const LweSecretKey& sk, const LweCiphertext& ct) {
  uint32_t pt = 0;
  e.check(tfhe_lwe_decrypt_batch(e.raw(), sk.data.data(), sk.data.size(), ct.data.data(), 1, &pt));
  return pt;
}

// encrypt_glwe_zero glwe.rs:190-209 (draw order: masks, then errors)
template <class Rng>
void fill_glwe_samples(const TfheParams& p, Rng& rng, uint32_t* row) {
  const size_t N = p.degree(), k = p.glwe_dimension;
  sample_uniform_slice(rng, row, k * N);
  sample_gaussian_slice(p.glwe_std_dev, rng, row + k * N, N);
}
template <class Rng>
GlweCiphertext encrypt_glwe_zero(Engine& e, const GlweSecretKey& sk, Rng& rng) {
  const TfheParams& p = e.params();
  GlweCiphertext ct{std::vector<uint32_t>((p.glwe_dimension + 1) * p.degree())};
  fill_glwe_samples(p, rng, ct.data.data());
  e.check(tfhe_glwe_encrypt_zero_batch(e.raw(), sk.data.data(), ct.data.data(), 1));
  return ct;
}
// encrypt_glwe_plaintext glwe.rs:211-230: message polynomial (encoded) added to the body
template <class Rng>
GlweCiphertext encrypt_glwe_plaintext(Engine& e, const std::vector<uint32_t>& plaintext, const GlweSecretKey& sk,
                                      Rng& rng) {
  const TfheParams& p = e.params();
  if (plaintext.size() != p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "plaintext shape");
  GlweCiphertext ct = encrypt_glwe_zero(e, sk, rng);
  uint32_t* body = ct.data.data() + p.glwe_dimension * p.degree();
  for (size_t i = 0; i < p.degree(); ++i) body[i] += plaintext[i];
  return ct;
}
// decrypt_glwe_ciphertext glwe.rs:245-265 -> encoded plaintext polynomial
inline std::vector<uint32_t> decrypt_glwe_ciphertext(Engine& e, const GlweSecretKey& sk, const GlweCiphertext& ct) {
  std::vector<uint32_t> pt(e.params().degree());
  e.check(tfhe_glwe_decrypt_batch(e.raw(), sk.data.data(), ct.data.data(), 1, pt.data()));
  return pt;
}
// encrypt_ggsw_plaintext ggsw.rs:76-130
template <class Rng>
GgswCiphertext encrypt_ggsw_plaintext(Engine& e, uint32_t message, const GlweSecretKey& sk, Rng& rng) {
  const TfheParams& p = e.params();
  const size_t row_words = (p.glwe_dimension + 1) * p.degree();
  GgswCiphertext g{std::vector<uint32_t>(p.ggsw_rows() * row_words)};
  for (size_t r = 0; r < p.ggsw_rows(); ++r) fill_glwe_samples(p, rng, g.data.data() + r * row_words);
  e.check(tfhe_ggsw_encrypt_batch(e.raw(), sk.data.data(), &message, g.data.data(), 1));
  return g;
}
// KeySwitchingKey::generate_ksk key_switching.rs:20-60 (the engine's ks_decomposer)
template <class Rng>
KeySwitchingKey generate_ksk(Engine& e, const LweSecretKey& from_lwe_sk, const LweSecretKey& to_lwe_sk,
                             double to_std_dev, Rng& rng) {
  const size_t to_n = to_lwe_sk.data.size();
  const size_t rows = from_lwe_sk.data.size() * e.params().ks_decomposer.levels;
  KeySwitchingKey ksk{std::vector<uint32_t>(rows * (to_n + 1))};
  for (size_t r = 0; r < rows; ++r) {  // encrypt_lwe_zero lwe.rs:117-136: error, then mask
    uint32_t* row = ksk.data.data() + r * (to_n + 1);
    sample_gaussian_slice(to_std_dev, rng, row + to_n, 1);
    sample_uniform_slice(rng, row, to_n);
  }
  e.check(tfhe_generate_ksk(e.raw(), from_lwe_sk.data.data(), from_lwe_sk.data.size(), to_lwe_sk.data.data(),
                            to_n, ksk.data.data()));
  return ksk;
}
// ---- packing key switch (tfhe_hip.h: many LWE results into one GLWE) ----
// These wrappers run on the engine's first device only (Engine::raw()): the packing key is not replicated over a pool.
// (from_dimension * l_ks, k+1, N): row i*l_ks + l encrypts from_sk[i] * g_l under the GLWE key
struct PackingKey {
  std::vector<uint32_t> data;
  size_t from_dimension = 0;
};
template <class Rng>
PackingKey generate_packing_key(Engine& e, const LweSecretKey& from_lwe_sk, const GlweSecretKey& glwe_sk, Rng& rng) {
  const TfheParams& p = e.params();
  const size_t row_words = (p.glwe_dimension + 1) * p.degree();
  const size_t rows = from_lwe_sk.data.size() * p.ks_decomposer.levels;
  PackingKey pk{std::vector<uint32_t>(rows * row_words), from_lwe_sk.data.size()};
  for (size_t r = 0; r < rows; ++r) fill_glwe_samples(p, rng, pk.data.data() + r * row_words);
  e.check(tfhe_generate_packing_key(e.raw(), from_lwe_sk.data.data(), from_lwe_sk.data.size(), glwe_sk.data.data(),
                                    pk.data.data()));
  return pk;
}
// TFHE_ERR_EXACTNESS where the engine's backend cannot pack exactly under the KS decomposer
inline void load_packing_key(Engine& e, const PackingKey& pk) {
  const TfheParams& p = e.params();
  if (pk.data.size() != pk.from_dimension * p.ks_decomposer.levels * (p.glwe_dimension + 1) * p.degree())
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "packing key shape");
  e.check(tfhe_load_packing_key(e.raw(), pk.data.data(), pk.from_dimension));
}
// up to N ciphertexts under the packing key's LWE key -> one GLWE whose coefficient j decrypts to what cts[j] does
inline GlweCiphertext pack_lwe(Engine& e, const std::vector<LweCiphertext>& cts) {
  const TfheParams& p = e.params();
  if (cts.empty() || cts.size() > p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "1 .. N ciphertexts per GLWE");
  size_t from_dimension = 0;
  int st = tfhe_packing_key_dimension(e.raw(), &from_dimension);
  if (st != TFHE_OK) throw TfheError(st, "pack_lwe: load a packing key first");
  const size_t width = from_dimension + 1;  // what the ABI reads per ciphertext
  std::vector<uint32_t> in(cts.size() * width);
  for (size_t j = 0; j < cts.size(); ++j) {
    if (cts[j].data.size() != width) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
    std::copy(cts[j].data.begin(), cts[j].data.end(), in.begin() + j * width);
  }
  GlweCiphertext out{std::vector<uint32_t>((p.glwe_dimension + 1) * p.degree())};
  e.check(tfhe_pack_lwe_batch(e.raw(), in.data(), 1, cts.size(), out.data.data()));
  return out;
}
// ---- CMUX tree and encrypted table lookup (tfhe_hip.h states the operations; first device only, like packing) ----
// GGSW encryptions of the `depth` address bits, least significant first: selector i of cmux_tree / table_lookup
template <class Rng>
std::vector<GgswCiphertext> encrypt_address(Engine& e, uint64_t address, size_t depth, const GlweSecretKey& sk, Rng& rng) {
  if (depth == 0 || depth > 63 || (address >> depth) != 0) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "address below 2^depth, depth 1..63");
  std::vector<GgswCiphertext> out;
  for (size_t i = 0; i < depth; ++i) out.push_back(encrypt_ggsw_plaintext(e, (uint32_t)((address >> i) & 1u), sk, rng));
  return out;
}
inline std::vector<uint32_t> flatten_selectors(const TfheParams& p, const std::vector<GgswCiphertext>& selectors) {
  const size_t words = p.ggsw_rows() * (p.glwe_dimension + 1) * p.degree();
  std::vector<uint32_t> flat(selectors.size() * words);
  for (size_t i = 0; i < selectors.size(); ++i) {
    if (selectors[i].data.size() != words) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GGSW shape");
    std::copy(selectors[i].data.begin(), selectors[i].data.end(), flat.begin() + i * words);
  }
  return flat;
}
// Tree(C_0 .. C_{d-1}; leaves): 2^d leaves, the result is leaf sum_i b_i 2^i where C_i encrypts b_i
inline GlweCiphertext cmux_tree(Engine& e, const std::vector<GgswCiphertext>& selectors, const std::vector<GlweCiphertext>& leaves) {
  const TfheParams& p = e.params();
  const size_t depth = selectors.size(), glwe = (p.glwe_dimension + 1) * p.degree();
  if (depth == 0 || depth > 20 || leaves.size() != (size_t)1 << depth) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "2^depth leaves, depth 1..20");
  const std::vector<uint32_t> sel = flatten_selectors(p, selectors);
  std::vector<uint32_t> in(leaves.size() * glwe);
  for (size_t i = 0; i < leaves.size(); ++i) {
    if (leaves[i].data.size() != glwe) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE shape");
    std::copy(leaves[i].data.begin(), leaves[i].data.end(), in.begin() + i * glwe);
  }
  GlweCiphertext out{std::vector<uint32_t>(glwe)};
  e.check(tfhe_cmux_tree(e.raw(), sel.data(), 1, depth, in.data(), 1, 1, out.data.data()));
  return out;
}
// table[address] of a clear table of 2^depth un-encoded values < 2^log_p -> LWE of k N + 1 words under the flattened
// GLWE key (key_switch_lwe brings it to dimension n)
inline LweCiphertext table_lookup(Engine& e, const std::vector<GgswCiphertext>& selectors, const std::vector<uint32_t>& table) {
  const TfheParams& p = e.params();
  const size_t depth = selectors.size();
  if (depth == 0 || depth > p.glwe_poly_degree + 20 || table.size() != (size_t)1 << depth)
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "2^depth table entries, depth 1..log2 N + 20");
  const std::vector<uint32_t> sel = flatten_selectors(p, selectors);
  LweCiphertext out{std::vector<uint32_t>(p.glwe_dimension * p.degree() + 1)};
  e.check(tfhe_table_lookup(e.raw(), sel.data(), 1, depth, table.data(), 1, 1, out.data.data()));
  return out;
}
// ---- encrypted branching program (tfhe_hip.h states the operations; first device only) ----
// nodes in topological order, terminals [n_terminals][N] clear message words, outputs: references (terminal t -> t, node
// i -> n_terminals + i).  selectors[s] encrypts input bit s.  -> one LWE of k N + 1 words per output under the
// flattened GLWE key
inline std::vector<LweCiphertext> cmux_program(Engine& e, const std::vector<GgswCiphertext>& selectors,
                                               const std::vector<tfhe_program_node>& nodes, const std::vector<uint32_t>& terminals,
                                               const std::vector<uint32_t>& outputs) {
  const TfheParams& p = e.params();
  const size_t lwe = p.glwe_dimension * p.degree() + 1;
  if (terminals.empty() || terminals.size() % p.degree() != 0 || outputs.empty())
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "terminals of N words each and at least one output");
  const std::vector<uint32_t> sel = flatten_selectors(p, selectors);
  std::vector<uint32_t> flat(outputs.size() * lwe);
  e.check(tfhe_cmux_program(e.raw(), sel.data(), 1, selectors.size(), 1, nodes.data(), nodes.size(), terminals.data(),
                            terminals.size() / p.degree(), outputs.data(), outputs.size(), nullptr, flat.data()));
  std::vector<LweCiphertext> out;
  for (size_t i = 0; i < outputs.size(); ++i)
    out.push_back(LweCiphertext{std::vector<uint32_t>(flat.begin() + i * lwe, flat.begin() + (i + 1) * lwe)});
  return out;
}
// ---- DEMUX tree and encrypted table update (tfhe_hip.h states the operations; first device only) ----
// Demux(C_0 .. C_{d-1}; x): 2^d leaves, leaf sum_i b_i 2^i carries x and every other one an encryption of 0
inline std::vector<GlweCiphertext> demux_tree(Engine& e, const std::vector<GgswCiphertext>& selectors, const GlweCiphertext& x) {
  const TfheParams& p = e.params();
  const size_t depth = selectors.size(), glwe = (p.glwe_dimension + 1) * p.degree();
  if (depth == 0 || depth > 20 || x.data.size() != glwe) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "one GLWE, depth 1..20");
  const std::vector<uint32_t> sel = flatten_selectors(p, selectors);
  std::vector<uint32_t> flat(((size_t)1 << depth) * glwe);
  e.check(tfhe_demux_tree(e.raw(), sel.data(), 1, depth, x.data.data(), 1, flat.data(), 1, 0));
  std::vector<GlweCiphertext> leaves;
  for (size_t i = 0; i < (size_t)1 << depth; ++i)
    leaves.push_back(GlweCiphertext{std::vector<uint32_t>(flat.begin() + i * glwe, flat.begin() + (i + 1) * glwe)});
  return leaves;
}
// A table of 2^depth entries as table_write / table_lookup_glwe hold it: max(1, 2^depth / N) GLWEs, entry a in
// coefficient a mod N of GLWE a / N.  (A trivial GLWE of encoded values is a valid start: see tfhe_hip.h.)
inline size_t table_glwes(const TfheParams& p, size_t depth) {
  return (size_t)1 << (depth > p.glwe_poly_degree ? depth - p.glwe_poly_degree : 0);
}
// table[address] += value, obliviously; `value` holds the encoded value in coefficient 0 of its phase.  The write ADDS:
// to replace an entry write new - old (old = table_lookup_glwe, packed with pack_lwe of that one ciphertext).
inline void table_write(Engine& e, const std::vector<GgswCiphertext>& selectors, const GlweCiphertext& value,
                        std::vector<GlweCiphertext>& table) {
  const TfheParams& p = e.params();
  const size_t depth = selectors.size(), glwe = (p.glwe_dimension + 1) * p.degree();
  if (depth == 0 || depth > p.glwe_poly_degree + 20 || table.size() != table_glwes(p, depth) || value.data.size() != glwe)
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "max(1, 2^depth / N) table GLWEs, depth 1..log2 N + 20");
  const std::vector<uint32_t> sel = flatten_selectors(p, selectors);
  std::vector<uint32_t> flat(table.size() * glwe);
  for (size_t i = 0; i < table.size(); ++i) {
    if (table[i].data.size() != glwe) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE shape");
    std::copy(table[i].data.begin(), table[i].data.end(), flat.begin() + i * glwe);
  }
  e.check(tfhe_table_write(e.raw(), sel.data(), 1, depth, value.data.data(), flat.data(), 1, 1));
  for (size_t i = 0; i < table.size(); ++i) std::copy(flat.begin() + i * glwe, flat.begin() + (i + 1) * glwe, table[i].data.begin());
}
// table[address] of an encrypted table (table_write's layout) -> LWE of k N + 1 words under the flattened GLWE key
inline LweCiphertext table_lookup_glwe(Engine& e, const std::vector<GgswCiphertext>& selectors, const std::vector<GlweCiphertext>& table) {
  const TfheParams& p = e.params();
  const size_t depth = selectors.size(), glwe = (p.glwe_dimension + 1) * p.degree();
  if (depth == 0 || depth > p.glwe_poly_degree + 20 || table.size() != table_glwes(p, depth))
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "max(1, 2^depth / N) table GLWEs, depth 1..log2 N + 20");
  const std::vector<uint32_t> sel = flatten_selectors(p, selectors);
  std::vector<uint32_t> flat(table.size() * glwe);
  for (size_t i = 0; i < table.size(); ++i) {
    if (table[i].data.size() != glwe) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE shape");
    std::copy(table[i].data.begin(), table[i].data.end(), flat.begin() + i * glwe);
  }
  LweCiphertext out{std::vector<uint32_t>(p.glwe_dimension * p.degree() + 1)};
  e.check(tfhe_table_lookup_glwe(e.raw(), sel.data(), 1, depth, flat.data(), 1, 1, out.data.data()));
  return out;
}
// ---- rotation from a GLWE accumulator and the tree LUT (tfhe_hip.h states the operations; first device only) ----
// X^{-(b~ + rotation_offset)} acc, then the n CMUXes: the accumulator's words are taken as they are (already encoded)
inline GlweCiphertext blind_rotate_glwe(Engine& e, const LweCiphertext& ct, const GlweCiphertext& acc, size_t rotation_offset = 0) {
  const TfheParams& p = e.params();
  const size_t glwe = (p.glwe_dimension + 1) * p.degree();
  if (ct.data.size() != size_t(p.lwe_dimension) + 1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
  if (acc.data.size() != glwe) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE shape");
  if (rotation_offset >= 2 * p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "rotation_offset below 2N");
  GlweCiphertext out{std::vector<uint32_t>(glwe)};
  e.check(tfhe_blind_rotate_glwe_batch(e.raw(), ct.data.data(), 1, acc.data.data(), 1, rotation_offset, out.data.data()));
  return out;
}
// ... + sample_extract(.., 0) + key_switch_lwe (the reference's order): a bootstrap whose table the server cannot read
// when acc is a GLWE encryption of the encoded test vector
inline LweCiphertext bootstrap_glwe(Engine& e, const LweCiphertext& ct, const GlweCiphertext& acc, size_t rotation_offset = 0) {
  const TfheParams& p = e.params();
  if (ct.data.size() != size_t(p.lwe_dimension) + 1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
  if (acc.data.size() != (p.glwe_dimension + 1) * p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE shape");
  if (rotation_offset >= 2 * p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "rotation_offset below 2N");
  LweCiphertext out{std::vector<uint32_t>(ct.data.size())};
  e.check(tfhe_bootstrap_glwe_batch(e.raw(), ct.data.data(), 1, acc.data.data(), 1, rotation_offset, out.data.data()));
  return out;
}
// table[sum_t x_t B^t] of d = digits.size() encrypted digits below B = 2^log_p (digit 0 least significant), table of
// B^d un-encoded values < B: an ordinary LWE of n + 1 words.  Needs the bootstrapping key and a packing key from the
// flattened GLWE key (generate_packing_key(e, lwe_secret_key_from(glwe_sk), glwe_sk, rng)).
inline LweCiphertext tree_lut(Engine& e, const std::vector<LweCiphertext>& digits, const std::vector<uint32_t>& table) {
  const TfheParams& p = e.params();
  const size_t d = digits.size();
  if (d == 0 || d * p.log_p > 16 || table.size() != (size_t)1 << (d * p.log_p))
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "B^d table entries, d * log_p in 1..16");
  std::vector<const uint32_t*> ptrs(d);
  for (size_t t = 0; t < d; ++t) {
    if (digits[t].data.size() != size_t(p.lwe_dimension) + 1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
    ptrs[t] = digits[t].data.data();
  }
  LweCiphertext out{std::vector<uint32_t>(size_t(p.lwe_dimension) + 1)};
  e.check(tfhe_tree_lut_batch(e.raw(), ptrs.data(), d, 1, table.data(), 1, 1, out.data.data()));
  return out;
}
// ---- digit extraction and the wide LUT (tfhe_hip.h states the operations; first device only) ----
// (ciphertexts of n + 1 words: the reference's bootstrap order only, like the wrappers around them; the key-switch-first
// order's k N + 1 words go through the C ABI)
// ONE ciphertext of n + 1 words with phase v 2^lsb + e -> its `digits` digits of `digit_bits` bits at out_lsb, digit 0
// least significant; remainder (may be null) receives the input with the extracted bits cleared: the carry
inline std::vector<LweCiphertext> extract_digits(Engine& e, const LweCiphertext& ct, unsigned lsb, unsigned digit_bits, unsigned digits,
                                                 unsigned out_lsb, LweCiphertext* remainder = nullptr) {
  const size_t words = ct.data.size();
  if (words != size_t(e.params().lwe_dimension) + 1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
  if (digits == 0 || digits > 16) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "digits in 1..16");
  std::vector<LweCiphertext> out(digits, LweCiphertext{std::vector<uint32_t>(words)});
  std::vector<uint32_t*> ptrs(digits);
  for (unsigned t = 0; t < digits; ++t) ptrs[t] = out[t].data.data();
  if (remainder) remainder->data.assign(words, 0u);
  e.check(tfhe_extract_digits_batch(e.raw(), ct.data.data(), 1, lsb, digit_bits, digits, out_lsb, ptrs.data(),
                                    remainder ? remainder->data.data() : nullptr));
  return out;
}
// T[v] of the d log_p low bits v of ONE encrypted value (phase v 2^lsb + e): table holds B^d un-encoded entries
inline LweCiphertext wide_lut(Engine& e, const LweCiphertext& ct, unsigned lsb, size_t d, const std::vector<uint32_t>& table) {
  const TfheParams& p = e.params();
  if (d == 0 || d * p.log_p > 16 || table.size() != (size_t)1 << (d * p.log_p))
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "B^d table entries, d * log_p in 1..16");
  if (ct.data.size() != size_t(p.lwe_dimension) + 1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
  LweCiphertext out{std::vector<uint32_t>(size_t(p.lwe_dimension) + 1)};
  e.check(tfhe_wide_lut_batch(e.raw(), ct.data.data(), 1, lsb, d, table.data(), 1, 1, out.data.data()));
  return out;
}
// ---- radix integers (tfhe_hip.h states the operations; first device only) ----
// A radix integer is `blocks` ciphertexts of n + 1 words back to back, block 0 least significant (the reference's bootstrap
// order only, like the wrappers above).
struct RadixCiphertext {
  size_t blocks = 0;
  std::vector<uint32_t> data;  // [blocks][n + 1]
};
// blocks of any value below 2^log_p -> the clean integer of the same value: 3 + ceil(log2(blocks - 1)) bootstrap levels
inline RadixCiphertext radix_propagate(Engine& e, const RadixCiphertext& x) {
  if (x.blocks == 0 || x.data.size() != x.blocks * (size_t(e.params().lwe_dimension) + 1)) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "radix length");
  RadixCiphertext out{x.blocks, std::vector<uint32_t>(x.data.size())};
  e.check(tfhe_radix_propagate_batch(e.raw(), x.data.data(), 1, x.blocks, out.data.data()));
  return out;
}
// one level: out_j = tables[table_of_block[j]][wa a_j + wb b_j], tables holding un-encoded values below 2^log_p (b may be
// null: a univariate lookup); the operands block by block, unshifted
inline RadixCiphertext radix_map(Engine& e, const RadixCiphertext& a, uint32_t wa, const RadixCiphertext* b, uint32_t wb,
                                 const std::vector<uint32_t>& tables, const std::vector<uint32_t>& table_of_block) {
  const size_t width = size_t(e.params().lwe_dimension) + 1, P = size_t(1) << e.params().log_p;
  if (a.blocks == 0 || a.data.size() != a.blocks * width || table_of_block.size() != a.blocks || tables.empty() || tables.size() % P != 0 ||
      (b && (b->blocks != a.blocks || b->data.size() != a.data.size())))
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "radix_map: operands of equal length, tables [count][2^log_p], one table index per block");
  RadixCiphertext out{a.blocks, std::vector<uint32_t>(a.data.size())};
  e.check(tfhe_radix_map_batch(e.raw(), a.data.data(), a.blocks, wa, 0, -1, b ? b->data.data() : nullptr, b ? b->blocks : 0, wb, 0, -1, 1,
                               a.blocks, tables.data(), tables.size() / P, table_of_block.data(), out.data.data()));
  return out;
}
// clean a, b of equal length and a predicate TFHE_RADIX_EQ .. TFHE_RADIX_GE -> one block in {0, 1}
inline LweCiphertext radix_compare(Engine& e, const RadixCiphertext& a, const RadixCiphertext& b, unsigned predicate) {
  const size_t width = size_t(e.params().lwe_dimension) + 1;
  if (a.blocks == 0 || a.blocks != b.blocks || a.data.size() != a.blocks * width || b.data.size() != a.data.size())
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "radix_compare: two integers of equal length");
  LweCiphertext out{std::vector<uint32_t>(width)};
  e.check(tfhe_radix_compare_batch(e.raw(), a.data.data(), b.data.data(), 1, a.blocks, predicate, out.data.data()));
  return out;
}
// ---- seeded ciphertexts and compressed keys (tfhe_hip.h states the generator, the layouts and the security rule) ----
// A seeded object is a seed and the bodies; the masks are G(seed, domain) (tfhe_seed_words).  NEVER use one
// (key, domain, stream) for two objects under the same secret key.
struct SeededLweRows {
  tfhe_seed seed{};
  size_t dimension = 0;
  std::vector<uint32_t> bodies;  // [rows]
};
struct SeededGlweRows {
  tfhe_seed seed{};
  std::vector<uint32_t> bodies;  // [rows][N]
};
// G(seed, domain)[first_word .. first_word + count): host code, no engine
inline std::vector<uint32_t> seed_words(const tfhe_seed& seed, uint32_t domain, uint64_t first_word, size_t count) {
  std::vector<uint32_t> out(count);
  if (int st = tfhe_seed_words(&seed, domain, first_word, count, out.data())) throw TfheError(st, "seed_words: the word range must stay within 2^36");
  return out;
}
// rows [first_row, first_row + rows) of the seeded object -> [rows][dimension + 1] / [rows][k+1][N]
inline std::vector<uint32_t> expand_lwe_rows(Engine& e, const SeededLweRows& x, uint64_t first_row = 0) {
  std::vector<uint32_t> out(x.bodies.size() * (x.dimension + 1));
  e.check(tfhe_expand_lwe_rows(e.raw(), &x.seed, x.bodies.data(), first_row, x.bodies.size(), x.dimension, out.data()));
  return out;
}
inline std::vector<uint32_t> expand_glwe_rows(Engine& e, const SeededGlweRows& x, uint64_t first_row = 0) {
  const size_t n = e.params().degree(), rows = x.bodies.size() / n;
  if (rows == 0 || x.bodies.size() != rows * n) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "expand_glwe_rows: bodies [rows][N]");
  std::vector<uint32_t> out(rows * (e.params().glwe_dimension + 1) * n);
  e.check(tfhe_expand_glwe_rows(e.raw(), &x.seed, x.bodies.data(), first_row, rows, out.data()));
  return out;
}
// the bodies of full rows
inline std::vector<uint32_t> compress_lwe_rows(Engine& e, const std::vector<uint32_t>& lwe, size_t dimension) {
  const size_t rows = lwe.size() / (dimension + 1);
  if (rows == 0 || lwe.size() != rows * (dimension + 1)) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "compress_lwe_rows: lwe [rows][dimension + 1]");
  std::vector<uint32_t> out(rows);
  e.check(tfhe_compress_lwe_rows(e.raw(), lwe.data(), rows, dimension, out.data()));
  return out;
}
inline std::vector<uint32_t> compress_glwe_rows(Engine& e, const std::vector<uint32_t>& glwe) {
  const size_t n = e.params().degree(), row = (e.params().glwe_dimension + 1) * n, rows = glwe.size() / row;
  if (rows == 0 || glwe.size() != rows * row) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "compress_glwe_rows: glwe [rows][k+1][N]");
  std::vector<uint32_t> out(rows * n);
  e.check(tfhe_compress_glwe_rows(e.raw(), glwe.data(), rows, out.data()));
  return out;
}
// the key from its seeded form: bsk bodies [n][(k+1)l][N], ksk bodies [kN l_ks] of dimension n (first device only)
inline void load_bootstrapping_key_seeded(Engine& e, const SeededGlweRows& bsk, const SeededLweRows& ksk) {
  const TfheParams& p = e.params();
  if (bsk.bodies.size() != size_t(p.lwe_dimension) * p.ggsw_rows() * p.degree() || ksk.dimension != p.lwe_dimension ||
      ksk.bodies.size() != p.lwe_dimension_post_pbs() * p.ks_decomposer.levels)
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "load_bootstrapping_key_seeded: bsk bodies [n][(k+1)l][N], ksk bodies [kN l_ks] of dimension n");
  e.check(tfhe_load_bootstrapping_key_seeded(e.raw(), &bsk.seed, bsk.bodies.data(), &ksk.seed, ksk.bodies.data()));
}
// bootstrap() of seeded inputs (rows first_row .. of the seed, the reference's bootstrap order: dimension n)
inline std::vector<LweCiphertext> bootstrap_seeded(Engine& e, const SeededLweRows& x, const std::vector<uint32_t>& test_vector_poly,
                                                   uint64_t first_row = 0) {
  const size_t width = size_t(e.params().lwe_dimension) + 1, batch = x.bodies.size();
  if (batch == 0 || x.dimension + 1 != width || test_vector_poly.size() != e.params().degree())
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "bootstrap_seeded: seeded rows of dimension n and one test vector [N]");
  std::vector<uint32_t> flat(batch * width);
  e.check(tfhe_bootstrap_batch_seeded(e.raw(), &x.seed, first_row, x.bodies.data(), batch, test_vector_poly.data(), 1, flat.data()));
  std::vector<LweCiphertext> out(batch);
  for (size_t i = 0; i < batch; ++i) out[i].data.assign(flat.begin() + i * width, flat.begin() + (i + 1) * width);
  return out;
}
// ---- encrypted dense layers (tfhe_hip.h states the operations; first device only) ----
// Dense(W, bias; x) for ONE query: x holds the I input ciphertexts (all of one length), weights [O][I] row-major int32,
// bias [O] already ENCODED words or empty -> O ciphertexts of that length, out[o] = sum_i W[o][i] x[i] (+ bias[o] on the body)
inline std::vector<LweCiphertext> dense(Engine& e, const std::vector<LweCiphertext>& x, const std::vector<int32_t>& weights,
                                        const std::vector<uint32_t>& bias = {}) {
  const size_t inputs = x.size();
  if (inputs == 0 || weights.empty() || weights.size() % inputs != 0) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "weights [O][I]");
  const size_t outputs = weights.size() / inputs, words = x[0].data.size();
  if (!bias.empty() && bias.size() != outputs) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "bias [O]");
  std::vector<uint32_t> flat;
  flat.reserve(inputs * words);
  for (const LweCiphertext& ct : x) {
    if (ct.data.size() != words) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
    flat.insert(flat.end(), ct.data.begin(), ct.data.end());
  }
  std::vector<uint32_t> res(outputs * words);
  e.check(tfhe_lwe_dense_batch(e.raw(), flat.data(), 1, inputs, weights.data(), bias.empty() ? nullptr : bias.data(), outputs, words,
                               res.data()));
  std::vector<LweCiphertext> out;
  for (size_t o = 0; o < outputs; ++o)
    out.push_back(LweCiphertext{std::vector<uint32_t>(res.begin() + o * words, res.begin() + (o + 1) * words)});
  return out;
}
// a whole layer for ONE query: out[o] = bootstrap(dense(x)[o]; test vector o mod tv_count); test_vectors holds one or O
// un-encoded test vectors of N words (construct_test_from_lut); ciphertexts of n + 1 words
inline std::vector<LweCiphertext> dense_bootstrap(Engine& e, const std::vector<LweCiphertext>& x, const std::vector<int32_t>& weights,
                                                  const std::vector<uint32_t>& bias, const std::vector<uint32_t>& test_vectors) {
  const TfheParams& p = e.params();
  const size_t inputs = x.size(), words = size_t(p.lwe_dimension) + 1;
  if (inputs == 0 || weights.empty() || weights.size() % inputs != 0) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "weights [O][I]");
  const size_t outputs = weights.size() / inputs;
  if (!bias.empty() && bias.size() != outputs) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "bias [O]");
  if (test_vectors.size() != p.degree() && test_vectors.size() != outputs * p.degree())
    throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "one or O test vectors of N words");
  std::vector<uint32_t> flat;
  flat.reserve(inputs * words);
  for (const LweCiphertext& ct : x) {
    if (ct.data.size() != words) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
    flat.insert(flat.end(), ct.data.begin(), ct.data.end());
  }
  std::vector<uint32_t> res(outputs * words);
  e.check(tfhe_dense_bootstrap_batch(e.raw(), flat.data(), 1, inputs, weights.data(), bias.empty() ? nullptr : bias.data(), outputs,
                                     test_vectors.data(), test_vectors.size() / p.degree(), res.data()));
  std::vector<LweCiphertext> out;
  for (size_t o = 0; o < outputs; ++o)
    out.push_back(LweCiphertext{std::vector<uint32_t>(res.begin() + o * words, res.begin() + (o + 1) * words)});
  return out;
}
// ---- encrypted convolutions (tfhe_hip.h states the operation; first device only) ----
// A prepared set of clear weight polynomials: weights [O][C][N] row-major int32, |w| small enough for the backend
// (TFHE_ERR_EXACTNESS with the reason otherwise).  Move-only; released with the object.
class PolyWeights {
 public:
  PolyWeights(Engine& e, const std::vector<int32_t>& weights, size_t outputs, size_t channels) {
    if (outputs == 0 || channels == 0 || weights.size() != outputs * channels * e.params().degree())
      throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "weights [O][C][N]");
    e.check(tfhe_prepare_poly_weights(e.raw(), weights.data(), outputs, channels, &w_));
  }
  PolyWeights(const PolyWeights&) = delete;
  PolyWeights& operator=(const PolyWeights&) = delete;
  PolyWeights(PolyWeights&& o) noexcept : w_(o.w_) { o.w_ = nullptr; }
  ~PolyWeights() { tfhe_poly_weights_destroy(w_); }
  const tfhe_poly_weights* raw() const { return w_; }
  size_t outputs() const { return info().outputs; }
  size_t channels() const { return info().channels; }
  unsigned weight_bits() const { return info().weight_bits; }
  unsigned rows_per_pass() const { return info().rows_per_pass; }

 private:
  struct Info {
    size_t outputs = 0, channels = 0;
    unsigned weight_bits = 0, rows_per_pass = 0;
  };
  Info info() const {
    Info i;
    (void)tfhe_poly_weights_info(w_, &i.outputs, &i.channels, &i.weight_bits, &i.rows_per_pass);
    return i;
  }
  tfhe_poly_weights* w_ = nullptr;
};
// Conv(W, bias; x) for ONE query: x holds the C input ciphertexts, bias [O][N] already ENCODED words or empty -> O
// ciphertexts, out[o] = sum_c W[o][c](X) * x[c] (+ bias[o] on the body), negacyclic, wrapping
inline std::vector<GlweCiphertext> glwe_conv(Engine& e, const std::vector<GlweCiphertext>& x, const PolyWeights& weights,
                                             const std::vector<uint32_t>& bias = {}) {
  const size_t glwe = size_t(e.params().glwe_dimension + 1) * e.params().degree(), outputs = weights.outputs();
  if (x.size() != weights.channels()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "one ciphertext per channel");
  if (!bias.empty() && bias.size() != outputs * e.params().degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "bias [O][N]");
  std::vector<uint32_t> flat;
  flat.reserve(x.size() * glwe);
  for (const GlweCiphertext& ct : x) {
    if (ct.data.size() != glwe) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE length");
    flat.insert(flat.end(), ct.data.begin(), ct.data.end());
  }
  std::vector<uint32_t> res(outputs * glwe);
  e.check(tfhe_glwe_conv_batch(e.raw(), flat.data(), 1, weights.raw(), bias.empty() ? nullptr : bias.data(), res.data()));
  std::vector<GlweCiphertext> out;
  for (size_t o = 0; o < outputs; ++o)
    out.push_back(GlweCiphertext{std::vector<uint32_t>(res.begin() + o * glwe, res.begin() + (o + 1) * glwe)});
  return out;
}
// sample_extract at every index of the list (each below N), in the list's order
inline std::vector<LweCiphertext> sample_extract_indices(Engine& e, const GlweCiphertext& glwe, const std::vector<uint32_t>& indices) {
  const size_t words = e.params().lwe_dimension_post_pbs() + 1;
  std::vector<uint32_t> res(indices.size() * words);
  e.check(tfhe_sample_extract_indices(e.raw(), glwe.data.data(), 1, indices.data(), indices.size(), res.data()));
  std::vector<LweCiphertext> out;
  for (size_t i = 0; i < indices.size(); ++i)
    out.push_back(LweCiphertext{std::vector<uint32_t>(res.begin() + i * words, res.begin() + (i + 1) * words)});
  return out;
}
// ---- GLWE key switching and automorphisms X -> X^t (tfhe_hip.h states the operation; first device only) ----
// sigma_t of a binary GLWE key [k][N] -> [k][N] with entries in {-1, 0, 1}: the from_polys of the automorphism key for t
inline std::vector<int32_t> glwe_sk_automorphism(const TfheParams& p, const std::vector<uint32_t>& glwe_sk, size_t t) {
  if (glwe_sk.size() != size_t(p.glwe_dimension) * p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE key [k][N]");
  std::vector<int32_t> out(glwe_sk.size());
  const int st = tfhe_glwe_sk_automorphism(glwe_sk.data(), p.glwe_dimension, p.glwe_poly_degree, t, out.data());
  if (st != TFHE_OK) throw TfheError(st, "glwe_sk_automorphism: a binary key and an odd t in [1, 2N)");
  return out;
}
// A prepared switch key.  `samples` [k l_ks][k+1][N]: pre-filled row by row like encrypt_glwe_zero (uniform masks, errors
// in the body) and completed here for from_polys [k][N] (entries in {-1, 0, 1}) and glwe_sk [k][N]; or an already
// generated key.  TFHE_ERR_EXACTNESS with the reason where the backend refuses a packing key.  Move-only; released with
// the object, before its engine.
class GlweSwitchKey {
 public:
  GlweSwitchKey(Engine& e, const std::vector<int32_t>& from_polys, const std::vector<uint32_t>& glwe_sk, std::vector<uint32_t> samples) {
    const size_t kn = size_t(e.params().glwe_dimension) * e.params().degree();
    if (from_polys.size() != kn || glwe_sk.size() != kn) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "from_polys and glwe_sk [k][N]");
    check_words(e, samples);
    e.check(tfhe_generate_glwe_switch_key(e.raw(), from_polys.data(), glwe_sk.data(), samples.data()));
    e.check(tfhe_prepare_glwe_switch_key(e.raw(), samples.data(), &key_));
  }
  GlweSwitchKey(Engine& e, const std::vector<uint32_t>& key) {
    check_words(e, key);
    e.check(tfhe_prepare_glwe_switch_key(e.raw(), key.data(), &key_));
  }
  GlweSwitchKey(const GlweSwitchKey&) = delete;
  GlweSwitchKey& operator=(const GlweSwitchKey&) = delete;
  GlweSwitchKey(GlweSwitchKey&& o) noexcept : key_(o.key_) { o.key_ = nullptr; }
  ~GlweSwitchKey() { tfhe_glwe_switch_key_destroy(key_); }
  const tfhe_glwe_switch_key* raw() const { return key_; }

 private:
  static void check_words(Engine& e, const std::vector<uint32_t>& key) {
    const TfheParams& p = e.params();
    if (key.size() != size_t(p.glwe_dimension) * p.ks_decomposer.levels * (p.glwe_dimension + 1) * p.degree())
      throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "switch key [k l_ks][k+1][N]");
  }
  tfhe_glwe_switch_key* key_ = nullptr;
};
// Auto_t(ct; key) (+ ct with add_input): X -> X^t and the switch back to the engine's key, for ONE ciphertext
inline GlweCiphertext glwe_automorphism(Engine& e, const GlweCiphertext& ct, size_t t, const GlweSwitchKey& key, bool add_input = false) {
  if (ct.data.size() != size_t(e.params().glwe_dimension + 1) * e.params().degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "GLWE length");
  GlweCiphertext out{std::vector<uint32_t>(ct.data.size())};
  e.check(tfhe_glwe_automorphism_batch(e.raw(), ct.data.data(), 1, t, key.raw(), add_input ? 1 : 0, out.data.data()));
  return out;
}
// the plain GLWE key switch (t = 1): from the key's source key to the engine's
inline GlweCiphertext glwe_key_switch(Engine& e, const GlweCiphertext& ct, const GlweSwitchKey& key) {
  return glwe_automorphism(e, ct, 1, key);
}
// ---- multi-bit blind rotation (tfhe_hip.h states the operation; first device only) ----
// A prepared multi-bit bootstrapping key for g in {2, 3, 4} key bits per step: from samples pre-filled like a GGSW batch
// (uniform masks, errors in the body) and completed here for lwe_sk [n] and glwe_sk [k][N]; or an already generated key.
// TFHE_ERR_UNSUPPORTED with the reason where the wide team is not offered.  Move-only; released with the object, before
// its engine.
class MultibitKey {
 public:
  MultibitKey(Engine& e, const std::vector<uint32_t>& lwe_sk, const std::vector<uint32_t>& glwe_sk, unsigned g, std::vector<uint32_t> samples) {
    const TfheParams& p = e.params();
    if (lwe_sk.size() != p.lwe_dimension || glwe_sk.size() != size_t(p.glwe_dimension) * p.degree())
      throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "lwe_sk [n] and glwe_sk [k][N]");
    check_words(e, g, samples);
    e.check(tfhe_generate_multibit_key(e.raw(), lwe_sk.data(), glwe_sk.data(), g, samples.data()));
    e.check(tfhe_prepare_multibit_key(e.raw(), samples.data(), g, &key_));
  }
  MultibitKey(Engine& e, const std::vector<uint32_t>& key, unsigned g) {
    check_words(e, g, key);
    e.check(tfhe_prepare_multibit_key(e.raw(), key.data(), g, &key_));
  }
  MultibitKey(const MultibitKey&) = delete;
  MultibitKey& operator=(const MultibitKey&) = delete;
  MultibitKey(MultibitKey&& o) noexcept : key_(o.key_) { o.key_ = nullptr; }
  ~MultibitKey() { tfhe_multibit_key_destroy(key_); }
  const tfhe_multibit_key* raw() const { return key_; }

 private:
  static void check_words(Engine& e, unsigned g, const std::vector<uint32_t>& key) {
    const TfheParams& p = e.params();
    if (g < 2 || g > 4) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "g must be 2, 3 or 4");
    const size_t groups = (size_t(p.lwe_dimension) + g - 1) / g, k1 = size_t(p.glwe_dimension) + 1;
    if (key.size() != groups * ((size_t(1) << g) - 1) * k1 * p.pbs_decomposer.levels * k1 * p.degree())
      throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "multi-bit key [ceil(n/g)][2^g - 1][(k+1) l][k+1][N]");
  }
  tfhe_multibit_key* key_ = nullptr;
};
// the multi-bit bootstrap of ONE ciphertext at the engine's boundary dimension against a clear test vector [N]
inline LweCiphertext multibit_bootstrap(Engine& e, const MultibitKey& key, const LweCiphertext& ct, const std::vector<uint32_t>& test_vector) {
  if (test_vector.size() != e.params().degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "test vector [N]");
  LweCiphertext out{std::vector<uint32_t>(ct.data.size())};
  e.check(tfhe_multibit_bootstrap_batch(e.raw(), key.raw(), ct.data.data(), 1, test_vector.data(), 1, out.data.data()));
  return out;
}
// the multi-bit blind rotation of ONE ciphertext of n + 1 words from a clear test vector [N] -> the GLWE accumulator
inline GlweCiphertext multibit_blind_rotate(Engine& e, const MultibitKey& key, const LweCiphertext& ct, const std::vector<uint32_t>& test_vector) {
  const TfheParams& p = e.params();
  if (ct.data.size() != size_t(p.lwe_dimension) + 1 || test_vector.size() != p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length / test vector [N]");
  GlweCiphertext out{std::vector<uint32_t>(size_t(p.glwe_dimension + 1) * p.degree())};
  e.check(tfhe_multibit_blind_rotate_batch(e.raw(), key.raw(), ct.data.data(), 1, test_vector.data(), 1, nullptr, 0, out.data.data(), nullptr));
  return out;
}
// ---- block-binary blind rotation (tfhe_hip.h states the operation; first device only) ----
// `block` key bits per decomposition on the engine's loaded, ordinary bootstrapping key: meaningful for an LWE secret with
// at most one 1 per block of `block` consecutive bits.  TFHE_ERR_EXACTNESS above block_rotate_max_block(),
// TFHE_ERR_UNSUPPORTED outside the fp64-fft backend at N = 512 / 1024.
inline unsigned block_rotate_max_block(Engine& e) {
  unsigned b = 0;
  e.check(tfhe_block_rotate_max_block(e.raw(), &b));
  return b;
}
// the block-binary bootstrap of ONE ciphertext at the engine's boundary dimension against a clear test vector [N]
inline LweCiphertext block_bootstrap(Engine& e, const LweCiphertext& ct, unsigned block, const std::vector<uint32_t>& test_vector) {
  if (test_vector.size() != e.params().degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "test vector [N]");
  LweCiphertext out{std::vector<uint32_t>(ct.data.size())};
  e.check(tfhe_block_bootstrap_batch(e.raw(), ct.data.data(), 1, block, test_vector.data(), 1, out.data.data()));
  return out;
}
// the block-binary blind rotation of ONE ciphertext of n + 1 words from a clear test vector [N] -> the GLWE accumulator
inline GlweCiphertext block_blind_rotate(Engine& e, const LweCiphertext& ct, unsigned block, const std::vector<uint32_t>& test_vector) {
  const TfheParams& p = e.params();
  if (ct.data.size() != size_t(p.lwe_dimension) + 1 || test_vector.size() != p.degree()) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length / test vector [N]");
  GlweCiphertext out{std::vector<uint32_t>(size_t(p.glwe_dimension + 1) * p.degree())};
  e.check(tfhe_block_blind_rotate_batch(e.raw(), ct.data.data(), 1, block, test_vector.data(), 1, nullptr, 0, out.data.data(), nullptr));
  return out;
}
// ---- multi-value bootstrapping (tfhe_hip.h states the operations; first device only) ----
// every lookup table of `luts` (tables x B un-encoded values, row-major) of ONE ciphertext of n + 1 words from one blind
// rotation (the reference's bootstrap order, like the neighbouring wrappers) -> one ciphertext per table
inline std::vector<LweCiphertext> multi_value_bootstrap(Engine& e, const LweCiphertext& ct, const std::vector<uint32_t>& luts) {
  const TfheParams& p = e.params();
  const size_t words = ct.data.size(), big_b = (size_t)1 << p.log_p;
  if (words != size_t(p.lwe_dimension) + 1) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "LWE length");
  if (luts.empty() || luts.size() % big_b != 0) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "tables of B = 2^log_p values");
  const size_t tables = luts.size() / big_b;
  std::vector<uint32_t> res(tables * words);
  e.check(tfhe_multi_value_bootstrap_batch(e.raw(), ct.data.data(), 1, luts.data(), 1, tables, res.data()));
  std::vector<LweCiphertext> out;
  for (size_t t = 0; t < tables; ++t)
    out.push_back(LweCiphertext{std::vector<uint32_t>(res.begin() + t * words, res.begin() + (t + 1) * words)});
  return out;
}
// the LWE ciphertexts (k N + 1 words) of coefficient 0 of (sum_m coeffs[t][m] X^positions[m]) * glwe, one per row t of
// coeffs (tables x positions.size(), row-major); positions distinct and below N
inline std::vector<LweCiphertext> glwe_sparse_extract(Engine& e, const GlweCiphertext& glwe, const std::vector<uint32_t>& positions,
                                                      const std::vector<int32_t>& coeffs) {
  const size_t words = e.params().lwe_dimension_post_pbs() + 1, terms = positions.size();
  if (terms == 0 || coeffs.empty() || coeffs.size() % terms != 0) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "rows of one coefficient per position");
  const size_t tables = coeffs.size() / terms;
  std::vector<uint32_t> res(tables * words);
  e.check(tfhe_glwe_sparse_extract_batch(e.raw(), glwe.data.data(), 1, positions.data(), terms, coeffs.data(), 1, tables, res.data()));
  std::vector<LweCiphertext> out;
  for (size_t t = 0; t < tables; ++t)
    out.push_back(LweCiphertext{std::vector<uint32_t>(res.begin() + t * words, res.begin() + (t + 1) * words)});
  return out;
}
// bootstrapping_key_gen bootstrapping.rs:23-56; the generated key is also installed in the engine.
// bmmp = true makes the key of the unrolled blind rotation instead (notes/BMMP Bootstrapping.md:22-24:
// GGSW(s s'), GGSW(s (1-s')), GGSW(s' (1-s)) per pair of key bits; N = 512, even n).
template <class Rng>
BootstrappingKey bootstrapping_key_gen(Engine& e, const LweSecretKey& lwe_secret_key,
                                       const GlweSecretKey& glwe_secret_key, Rng& rng, bool bmmp = false) {
  const TfheParams& p = e.params();
  const size_t n = p.lwe_dimension, row_words = (p.glwe_dimension + 1) * p.degree();
  const size_t ggsw_words = p.ggsw_rows() * row_words;
  const size_t ggsws = bmmp ? n / 2 * 3 : n;
  if (lwe_secret_key.data.size() != n) throw TfheError(TFHE_ERR_INVALID_ARGUMENT, "lwe secret key shape");
  std::vector<uint32_t> bsk(ggsws * ggsw_words);
  for (size_t r = 0; r < ggsws * p.ggsw_rows(); ++r) fill_glwe_samples(p, rng, bsk.data() + r * row_words);
  const size_t ks_rows = p.lwe_dimension_post_pbs() * p.ks_decomposer.levels;
  KeySwitchingKey ksk{std::vector<uint32_t>(ks_rows * (n + 1))};
  for (size_t r = 0; r < ks_rows; ++r) {
    uint32_t* row = ksk.data.data() + r * (n + 1);
    sample_gaussian_slice(p.lwe_std_dev, rng, row + n, 1);
    sample_uniform_slice(rng, row, n);
  }
  // (the pool entry point: generated on the first device, installed on EVERY device of the engine)
  e.check_pool((bmmp ? tfhe_pool_bootstrapping_key_gen_bmmp : tfhe_pool_bootstrapping_key_gen)(
      e.raw_pool(), lwe_secret_key.data.data(), glwe_secret_key.data.data(), bsk.data(), ksk.data.data(), 1));
  BootstrappingKey bk;
  bk.lwe_sk_ggsw_enc.reserve(ggsws);
  for (size_t i = 0; i < ggsws; ++i)
    bk.lwe_sk_ggsw_enc.push_back(
        GgswCiphertext{std::vector<uint32_t>(bsk.begin() + i * ggsw_words, bsk.begin() + (i + 1) * ggsw_words)});
  bk.ksk = std::move(ksk);
  return bk;
}

}  // namespace tfhe_amd
