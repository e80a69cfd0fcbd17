// capi.cpp -- implementation of the C ABI declared in include/tfhe_hip.h.
//
// Host-side only logic: parameter validation (mirrors what makes the reference panic), device
// memory management, key preparation and kernel sequencing.  No CPU implementation of the hot
// path lives here: without a GPU every compute entry point fails with TFHE_ERR_NO_DEVICE.
#include "context.h"
#include "passes.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <algorithm>
#include <string>
#include <vector>

namespace {

using namespace tfhe::host;  // fail, hip_fail, the sizes

// Bit just above the most significant limb: gadget factor of level i is 2^{top - log_base*(i+1)} and
// the lowest kept limb starts at top - log_base*levels.  Literal (reference, decomposer.rs:48-70 /
// ggsw.rs:98): limbs are counted from bit 0, so top = log_base*floor(32/log_base).  Aligned: 32.
u32 gadget_top(const tfhe_context* ctx, u32 log_base) {
  return ctx->aligned ? 32u : log_base * (32u / log_base);
}

// one workgroup per sample: the grid's x dimension is a 32-bit count
constexpr size_t kMaxBatch = 0x7FFFFFFFull;

int decomposer_validate(const tfhe_decomposer_params& d) {
  if (d.log_q != 32) return 1;                        // the reference is hard-typed to u32
  if (d.log_base == 0 || d.log_base >= 32) return 2;  // 1 << (log_base - 1), 1 << log_base
  if (d.levels == 0) return 3;
  if (d.log_base * d.levels > d.log_q) return 4;      // usize underflow, decomposer.rs:28
  if (d.levels > d.log_q / d.log_base) return 5;      // truncation loop never ends, :74-77
  return 0;
}

int reserve(tfhe_context* ctx, size_t batch) {
  if (batch <= ctx->ws_batch) return TFHE_OK;
  // every LWE buffer can hold either boundary dimension (n for the reference's PBS-then-KS order,
  // k*N for KS-then-PBS), so switching the order never reallocates
  const size_t n1 = std::max((size_t)ctx->params.lwe_dimension, (size_t)ctx->big_n) + 1;
  const size_t glwe = glwe_words(ctx);
  DeviceBuffer* bufs[] = {&ctx->d_lwe_in, &ctx->d_lwe_in2, &ctx->d_lwe_big, &ctx->d_lwe_out, &ctx->d_lwe_ks,
                          &ctx->d_glwe_a, &ctx->d_glwe_b,   &ctx->d_glwe_c,  &ctx->d_tv};
  const size_t sizes[] = {batch * n1, batch * n1, batch * n1, batch * n1, batch * n1,
                          batch * glwe, batch * glwe, batch * glwe, batch * ctx->N};
  // the old workspace is gone from here on: ws_batch claims nothing until all nine are there again
  ctx->ws_batch = 0;
  // all nine go before one comes back: the peak of a large batch regrowing is the new workspace, not old plus new
  for (DeviceBuffer* b : bufs) TFHE_TRY(b->resize(ctx, 0));
  for (int i = 0; i < 9; ++i) TFHE_TRY(bufs[i]->grow(ctx, sizes[i] * sizeof(u32)));
  ctx->ws_batch = batch;
  return TFHE_OK;
}

int check_ctx(tfhe_context* ctx) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
  return TFHE_OK;
}

// every pointer there and the count not 0, or the refusal `what`
int check_present(tfhe_context* ctx, std::initializer_list<const void*> ptrs, size_t count = 1,
                  const char* what = "null pointer / empty batch") {
  for (const void* p : ptrs)
    if (!p) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, what);
  if (count == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, what);
  return TFHE_OK;
}

// The pointers, the batch and the 1-or-batch count (`count_name` in the refusal) of a batched family.  The rotations
// and bootstraps name each failure and look at the grid limit first; the products (external product, CMUX) grew up with
// one text for null / empty and the count first, and their host forms without the grid limit (a batch beyond it fails
// in reserve()): a refusal's status, text and precedence are part of the ABI.
enum BatchFamily { kRotations, kProducts, kHostProducts };

int check_batch(tfhe_context* ctx, std::initializer_list<const void*> ptrs, size_t batch, size_t count,
                const char* count_name, BatchFamily family = kRotations) {
  const bool count_ok = count == 1 || count == batch;
  const std::string bad_count = std::string(count_name) + " must be 1 or batch";
  if (family != kRotations) {
    TFHE_TRY(check_present(ctx, ptrs, batch));
    if (!count_ok) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, bad_count);
    if (family == kProducts && batch > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch exceeds 2^31 - 1");
    return TFHE_OK;
  }
  TFHE_TRY(check_present(ctx, ptrs, 1, "null pointer"));
  if (batch == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "empty batch");
  if (batch > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch exceeds 2^31 - 1 (one workgroup per sample)");
  if (!count_ok) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, bad_count);
  return TFHE_OK;
}

// ---- staging of the host forms: copy in, the _device form, copy out, ONE synchronisation -- all on the context's stream
int upload(tfhe_context* ctx, u32* dev, const void* host, size_t words) {
  HIP_TRY(ctx, hipMemcpyAsync(dev, host, words * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
  return TFHE_OK;
}

int download(tfhe_context* ctx, void* host, const u32* dev, size_t words) {
  HIP_TRY(ctx, hipMemcpyAsync(host, dev, words * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
  return TFHE_OK;
}

// how a host form ends: its result comes back and the stream drains
int download_and_wait(tfhe_context* ctx, void* host, const u32* dev, size_t words) {
  TFHE_TRY(download(ctx, host, dev, words));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_OK;
}

// The small entry points stage in the context's scratch buffer (d_misc): segments of 32-bit words back to back, in the
// order given, unpadded.  (The forms whose operands have a buffer in the reserve() workspace stage there instead.)
class Staging {
 public:
  Staging(tfhe_context* ctx, std::vector<size_t> words) : ctx_(ctx), words_(std::move(words)) {}
  // grows the scratch buffer if the segments need it (synchronises only then); call first
  int reserve() {
    size_t total = 0;
    for (size_t w : words_) total += w;
    return ctx_->d_misc.grow(ctx_, total * sizeof(u32));
  }
  u32* operator[](size_t seg) const {
    u32* p = ctx_->d_misc.as<u32>();
    for (size_t i = 0; i < seg; ++i) p += words_[i];
    return p;
  }
  int upload(size_t seg, const void* host) const { return ::upload(ctx_, (*this)[seg], host, words_[seg]); }
  int download_and_wait(size_t seg, void* host) const { return ::download_and_wait(ctx_, host, (*this)[seg], words_[seg]); }

 private:
  tfhe_context* ctx_;
  std::vector<size_t> words_;
};

// A host form whose one buffer [words] goes in, is completed by the _device form, and comes back
template <class DeviceForm>
int in_place_host_form(tfhe_context* ctx, u32* host, size_t words, DeviceForm device_form) {
  Staging s(ctx, {words});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(0, host));
  TFHE_TRY(device_form(s[0]));
  return s.download_and_wait(0, host);
}

// Row s*levels + level of a key-switching key (key_switching.rs:36-45) or a packing key carries
// sk[s] * 2^{log_base*(l - (level+1))}, the KS decomposer's gadget factor of that level
std::vector<u32> gadget_factors(const tfhe_context* ctx, const u32* sk, size_t dimension) {
  const u32 levels = ctx->ks.levels, log_base = ctx->ks.log_base;
  const u32 top = gadget_top(ctx, log_base);
  std::vector<u32> factor(dimension * levels);
  for (size_t s = 0; s < dimension; ++s)
    for (u32 level = 0; level < levels; ++level)
      factor[s * levels + level] = (1u << (top - log_base * (level + 1))) * sk[s];
  return factor;
}

// The external product's parameters with the KS decomposer.  Read per call: the decomposer may have been re-aligned since
// the key was loaded (as for the KSK, the caller keeps them in step)
PbsParams packing_params(const tfhe_context* ctx) {
  PbsParams P = ctx->pbs;
  P.log_base = ctx->ks.log_base;
  P.levels = ctx->ks.levels;
  P.ignored_bits = ctx->ks.ignored_bits;
  P.first_shift = ctx->ks.first_shift;
  return P;
}

// Why this backend cannot sum `rows` products of digits of magnitude 2^lb with key words in the transform domain and lift
// the sum exactly, or "" if it can: every backend's exactness rule in its (rows, log_base) form -- the complex transform's
// FftField::error_bound(log N, rows, lb) < kMaxError, log2 rows + log N + lb + key_bits < exact_bits in the prime fields,
// and each field's kMaxRows / kSmallBits / kMaxLogBase.  The nouns name what the caller sums: the packing key switch
// the (k+1) l_ks rows of a slice in the KS base, the convolution the channels of a pass at the weights' magnitude.
struct ExactnessNouns {
  const char* base;  // what lb is
  const char* rows;  // what the rows are
  const char* unit;  // what is summed before a lift
};
std::string exactness_refusal(const tfhe_context* ctx, int rows, int lb, const ExactnessNouns& noun) {
  const tfhe_params& p = ctx->params;
  const double bits = std::log2((double)rows) + p.glwe_poly_degree + lb;
  auto prime = [&](const char* name, double key_bits, double exact_bits, int max_rows, int small_bits, int max_log_base) {
    char buf[256];
    if (lb > max_log_base || lb > small_bits) {
      std::snprintf(buf, sizeof buf, "%s: %s %d exceeds the backend's largest gadget base 2^%d", name, noun.base, lb,
                    std::min(max_log_base, small_bits));
      return std::string(buf);
    }
    if (rows > max_rows) {
      std::snprintf(buf, sizeof buf, "%s: %s = %d rows per %s exceed the backend's %d", name, noun.rows, rows, noun.unit, max_rows);
      return std::string(buf);
    }
    if (!(bits + key_bits < exact_bits)) {
      std::snprintf(buf, sizeof buf, "%s: a %s of %s = %d rows in base 2^%d needs %.2f bits, the field lifts %.2f", name, noun.unit,
                    noun.rows, rows, lb, bits + key_bits, exact_bits);
      return std::string(buf);
    }
    return std::string();
  };
  switch (ctx->field) {
    case launch::kFieldFp64:
      return prime("fp64-p42", FpField::key_bits(), FpField::exact_bits(), FpField::kMaxRows, FpField::kSmallBits, FpField::kMaxLogBase);
    case launch::kFieldFp49:
      return prime("fp64-p49", Fp49Field::key_bits(), Fp49Field::exact_bits(), Fp49Field::kMaxRows, Fp49Field::kSmallBits, Fp49Field::kMaxLogBase);
    case launch::kFieldGoldilocks:
      return prime("goldilocks", GlField::key_bits(), GlField::exact_bits(), GlField::kMaxRows, GlField::kSmallBits, GlField::kMaxLogBase);
    case launch::kFieldGoldilocksSplit:
      return prime("goldilocks-split", GlSplitField::key_bits(), GlSplitField::exact_bits(), GlSplitField::kMaxRows,
                   GlSplitField::kSmallBits, GlSplitField::kMaxLogBase);
    default: {
      char buf[256];
      if (lb > FftField::kMaxLogBase || lb > FftField::kSmallBits) {
        std::snprintf(buf, sizeof buf, "fp64-fft: %s %d exceeds FftField::kMaxLogBase = %d", noun.base, lb, FftField::kMaxLogBase);
        return std::string(buf);
      }
      if (rows > FftField::kMaxRows) {
        std::snprintf(buf, sizeof buf, "fp64-fft: %s = %d rows per %s exceed FftField::kMaxRows = %d", noun.rows, rows, noun.unit,
                      FftField::kMaxRows);
        return std::string(buf);
      }
      const double err = FftField::error_bound((int)p.glwe_poly_degree, rows, lb);
      if (!(err < FftField::kMaxError)) {
        std::snprintf(buf, sizeof buf, "fp64-fft: rounding bound %.4g of a %s of %d rows in base 2^%d is not below %.4g", err,
                      noun.unit, rows, lb, FftField::kMaxError);
        return std::string(buf);
      }
      return std::string();
    }
  }
}

// ---- timing spans: events 0/1 bracket a rotation, 2/3 a key switch (tfhe_last_kernel_ms)
enum Span { kRotationSpan = 0, kKeySwitchSpan = 2 };

int span_begin(tfhe_context* ctx, Span span) {
  ctx->ev_valid_mb = false;  // the events of a multi-bit rotation's launches (tfhe_multibit_last_kernel_ms) are reused
  if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev[span], ctx->stream));
  return TFHE_OK;
}

// alone: the call times this span only, the other one's events are stale (a bootstrap ends both and says so itself)
int span_end(tfhe_context* ctx, Span span, bool alone = true) {
  if (!ctx->timing) return TFHE_OK;
  HIP_TRY(ctx, hipEventRecord(ctx->ev[span + 1], ctx->stream));
  if (alone) {
    ctx->ev_valid_br = span == kRotationSpan;
    ctx->ev_valid_ks = span == kKeySwitchSpan;
  }
  return TFHE_OK;
}

// construct_test_from_lut: test_vector.rs:38-67
int test_from_lut(const tfhe_params* p, const u32* lut, size_t lut_len, u32* out) {
  const u32 plaintext_modulus = 1u << p->log_p;
  if (lut_len != plaintext_modulus) return TFHE_ERR_INVALID_ARGUMENT;  // assert! :41
  const size_t n = (size_t)1 << p->glwe_poly_degree;
  const size_t repetition = n / ((size_t)1 << p->log_p);
  std::vector<u32> tv;
  tv.reserve(repetition * lut_len);
  for (size_t v = 0; v < lut_len; ++v)
    for (size_t r = 0; r < repetition; ++r) tv.push_back(lut[v]);
  for (size_t i = 0; i < repetition / 2; ++i)
    if (tv[i] != 0) tv[i] = plaintext_modulus - tv[i];
  const size_t mid = repetition / 2, len = tv.size();
  for (size_t i = 0; i < len; ++i) out[i] = tv[(i + mid) % len];  // rotate_left(mid)
  return TFHE_OK;
}

int check_tv_host(tfhe_context* ctx, const u32* tv, size_t words) {
  // glwe.rs:144 assert!(*m < 1 << log_p)
  if (ctx->params.log_p >= 32) return TFHE_OK;
  const u32 lim = 1u << ctx->params.log_p;
  for (size_t i = 0; i < words; ++i)
    if (tv[i] >= lim)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "test vector value >= 2^log_p (glwe.rs:144)");
  return TFHE_OK;
}

// the blind rotation the loaded key calls for: bootstrapping.rs:79-105, or the unrolled loop of
// notes/BMMP Bootstrapping.md with a BMMP key
// Where a rotation's accumulator starts: the clear test vector(s) tv [tv_count][N], or (glwe) the GLWE ciphertext(s)
// tv [tv_count][k+1][N], already encoded, rotated by `offset` more (PbsParams::acc_glwe / acc_offset; not with a BMMP key:
// the entry points refuse that before they get here)
struct AccSource {
  bool glwe = false;
  u32 offset = 0;
  u32* state = nullptr;  // [batch][k+1][N] for the segments' accumulators instead of the context's workspace (tree LUT)
};

hipError_t enqueue_blind_rotate(tfhe_context* ctx, const u32* lwe_in, size_t batch, const u32* tv,
                                size_t tv_count, u32* glwe_out, u32* lwe_extracted, AccSource from = AccSource()) {
  if (ctx->bmmp)
    return launch::blind_rotate_bmmp(ctx->stream, ctx->field, ctx->pbs, ctx->d_tw.as(), lwe_in, batch, tv,
                                     tv_count == 1 ? 0 : ctx->N, ctx->d_bsk.as(), glwe_out, lwe_extracted);
  // accumulators between the launches of a segmented rotation: the caller's output, or the workspace (sized by reserve)
  u32* state = glwe_out ? glwe_out : from.state ? from.state : (batch <= ctx->ws_batch ? ctx->d_glwe_c.as<u32>() : nullptr);
  PbsParams P = ctx->pbs;
  P.acc_glwe = from.glwe ? 1u : 0u;
  P.acc_offset = from.offset;
  const size_t tv_words = from.glwe ? glwe_words(ctx) : (size_t)ctx->N;
  return launch::blind_rotate(ctx->stream, ctx->field, P, ctx->d_tw.as(), lwe_in, batch, tv, tv_count == 1 ? 0 : tv_words,
                              ctx->d_bsk.as(), glwe_out, lwe_extracted, state, &ctx->side, ctx->shape);
}

// Enqueue the whole PBS on device buffers: blind rotation (+ fused sample extract), key switch (bootstrapping.rs:58-120),
// or the key switch first.  d_lwe_big: [batch][k*N+1] scratch of the reference order (unused when the key switch comes first)
// rotate(br_in, br_out) enqueues the rotation with its sample extract: the loaded key's, or a multi-bit key's
template <class Rotate>
int enqueue_bootstrap_with(tfhe_context* ctx, const u32* d_lwe_in, size_t batch, u32* d_lwe_big, u32* d_lwe_out, Rotate rotate) {
  const u32* br_in = d_lwe_in;
  u32* br_out = d_lwe_big;
  if (ctx->timing) {  // next slot of the ring
    ctx->ev_slot = (ctx->ev_slot + 1) % tfhe_context::kTimingSlots;
    ctx->ev = ctx->ev_ring[ctx->ev_slot];
    ++ctx->timed_bootstraps;
  }
  auto key_switch = [&](const u32* in, u32* out) -> int {
    TFHE_TRY(span_begin(ctx, kKeySwitchSpan));
    HIP_TRY(ctx, launch::key_switch(ctx->stream, ctx->ks, ctx->big_n, ctx->params.lwe_dimension, in, batch, ctx->d_ksk.as<u32>(), out, ctx->d_ksk_matrix.as(), ctx->ks_path));
    return span_end(ctx, kKeySwitchSpan, false);
  };
  if (ctx->ks_first) {  // notes/TFHE.md:367-400: key switch k*N -> n, then PBS back to k*N
    TFHE_TRY(key_switch(d_lwe_in, ctx->d_lwe_ks.as<u32>()));
    br_in = ctx->d_lwe_ks.as<u32>();
    br_out = d_lwe_out;
  }
  TFHE_TRY(span_begin(ctx, kRotationSpan));
  HIP_TRY(ctx, rotate(br_in, br_out));
  TFHE_TRY(span_end(ctx, kRotationSpan, false));
  if (!ctx->ks_first) TFHE_TRY(key_switch(d_lwe_big, d_lwe_out));
  if (ctx->timing) ctx->ev_valid_br = ctx->ev_valid_ks = true;
  return TFHE_OK;
}

int enqueue_bootstrap(tfhe_context* ctx, const u32* d_lwe_in, size_t batch, const u32* d_tv,
                      size_t tv_count, u32* d_lwe_big, u32* d_lwe_out, AccSource from = AccSource()) {
  return enqueue_bootstrap_with(ctx, d_lwe_in, batch, d_lwe_big, d_lwe_out, [&](const u32* br_in, u32* br_out) {
    return enqueue_blind_rotate(ctx, br_in, batch, d_tv, tv_count, nullptr, br_out, from);
  });
}

// log2 of the worst-case |integer convolution value| one inverse transform has to lift:
// R * N * max|digit| (= B, decomposer.rs:54-63) * max|key operand|
double convolution_bits(const tfhe_params* p, double key_bits) {
  return std::log2((double)(p->glwe_dimension + 1) * p->pbs_decomposer.levels) + p->glwe_poly_degree +
         p->pbs_decomposer.log_base + key_bits;
}

template <class F>
int upload_twiddles(tfhe_context* ctx) {
  // (the complex transform has N/2 points: F::kLogShrink = 1)
  std::vector<typename F::elem> tw(ntt_twiddle_words((int)(ctx->N >> F::kLogShrink)));
  F::fill_twiddles((int)ctx->params.glwe_poly_degree - F::kLogShrink, tw.data());
  TFHE_TRY(ctx->d_tw.grow(ctx, tw.size() * sizeof(typename F::elem)));
  HIP_TRY(ctx, hipMemcpy(ctx->d_tw.as(), tw.data(), tw.size() * sizeof(typename F::elem), hipMemcpyHostToDevice));
  return TFHE_OK;
}

// the block-binary rotation's factor table (block_rotate.h::fill_block_roots), where that rotation is offered
int upload_block_roots(tfhe_context* ctx) {
  if (!launch::block_rotate_supported(ctx->field, ctx->params.glwe_poly_degree, ctx->params.glwe_dimension)) return TFHE_OK;
  std::vector<cplx> roots(block_root_words((int)ctx->params.glwe_poly_degree));
  fill_block_roots((int)ctx->params.glwe_poly_degree, roots.data());
  TFHE_TRY(ctx->d_block_roots.grow(ctx, roots.size() * sizeof(cplx)));
  HIP_TRY(ctx, hipMemcpy(ctx->d_block_roots.as(), roots.data(), roots.size() * sizeof(cplx), hipMemcpyHostToDevice));
  return TFHE_OK;
}

// The prepared bootstrapping key for `ggsws` GGSWs (reallocated when the other kind of key was loaded before: its
// footprint follows the key), the key-switching key and, where it is wanted, its matrix-path layout (allocated once:
// their sizes are the context's).  The caller has taken the old key out of service (have_key) before.
int ensure_key_buffers(tfhe_context* ctx, size_t ggsws, bool want_matrix) {
  ctx->bsk_ggsws = 0;
  TFHE_TRY(ctx->d_bsk.resize(ctx, prepared_bsk_bytes(ctx, ggsws)));
  ctx->bsk_ggsws = ggsws;
  TFHE_TRY(ctx->d_ksk.grow(ctx, ksk_words(ctx) * sizeof(u32)));
  if (want_matrix) TFHE_TRY(ctx->d_ksk_matrix.grow(ctx, ksk_matrix_bytes(ctx)));
  return TFHE_OK;
}

}  // namespace

namespace tfhe {
namespace host {

int adopt_prepared_key(tfhe_context* dst, const tfhe_context* src) {
  if (!dst || !src || !src->have_key) return fail(dst, TFHE_ERR_NO_KEY, "source context holds no key");
  if (std::memcmp(&dst->params, &src->params, sizeof(tfhe_params)) != 0 || dst->field != src->field ||
      dst->aligned != src->aligned)
    return fail(dst, TFHE_ERR_INVALID_PARAMS, "pool members must share parameters, backend and decomposer alignment");
  // from here on dst has NO key until the copies are enqueued: a failure half way must not leave it answering under the
  // key it held before
  dst->have_key = false;
  HIP_TRY(dst, hipSetDevice(dst->device));
  const size_t ggsws = src->bsk_ggsws;
  const size_t bsk_bytes = prepared_bsk_bytes(src, ggsws), ksk_bytes = ksk_words(src) * sizeof(u32);
  const size_t ksm_bytes = src->d_ksk_matrix.bytes();  // same parameters: admitted on both or neither
  TFHE_TRY(ensure_key_buffers(dst, ggsws, ksm_bytes != 0));
  if (dst->device == src->device) {
    HIP_TRY(dst, hipMemcpyAsync(dst->d_bsk.as(), src->d_bsk.as(), bsk_bytes, hipMemcpyDeviceToDevice, dst->stream));
    HIP_TRY(dst, hipMemcpyAsync(dst->d_ksk.as<u32>(), src->d_ksk.as<u32>(), ksk_bytes, hipMemcpyDeviceToDevice, dst->stream));
    if (ksm_bytes)
      HIP_TRY(dst, hipMemcpyAsync(dst->d_ksk_matrix.as(), src->d_ksk_matrix.as(), ksm_bytes, hipMemcpyDeviceToDevice, dst->stream));
  } else {
    // direct xGMI copies where the link allows peer access; hipMemcpyPeerAsync stages through the host otherwise
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dst->device, src->device) == hipSuccess && can) {
      hipError_t e = hipDeviceEnablePeerAccess(src->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return hip_fail(dst, e, "hipDeviceEnablePeerAccess");
      (void)hipGetLastError();
    }
    HIP_TRY(dst, hipMemcpyPeerAsync(dst->d_bsk.as(), dst->device, src->d_bsk.as(), src->device, bsk_bytes, dst->stream));
    HIP_TRY(dst, hipMemcpyPeerAsync(dst->d_ksk.as<u32>(), dst->device, src->d_ksk.as<u32>(), src->device, ksk_bytes, dst->stream));
    if (ksm_bytes)
      HIP_TRY(dst, hipMemcpyPeerAsync(dst->d_ksk_matrix.as(), dst->device, src->d_ksk_matrix.as(), src->device, ksm_bytes, dst->stream));
  }
  dst->have_key = true;
  dst->bmmp = src->bmmp;
  return TFHE_OK;
}

}  // namespace host
}  // namespace tfhe

extern "C" {

// The shipped library's string carries no '[': a dev build (TFHE_DEV_BUILD: the only kind that may compile a WRONG-BITS
// timing probe in, csrc/dev_switches.h), the rounding-margin probe build and one-shape / one-field builds all say so.
const char* tfhe_version(void) {
  return "tfhe-research_amd 0.5 (gfx950; exact backends: fp64-fft, fp64-p49, fp64-p42, goldilocks, goldilocks-split)"
#if defined(TFHE_DEV_BUILD)
         " [DEV BUILD: not for use"
#if TFHE_PROBE_HOT_KEY
         "; WRONG BITS: TFHE_PROBE_HOT_KEY"
#endif
#if TFHE_PROBE_NO_EXCHANGE_READS
         "; WRONG BITS: TFHE_PROBE_NO_EXCHANGE_READS"
#endif
#if TFHE_PROBE_NO_TRANSPOSE
         "; WRONG BITS: TFHE_PROBE_NO_TRANSPOSE"
#endif
#if TFHE_PROBE_NO_TEAM_SYNC
         "; WRONG BITS: TFHE_PROBE_NO_TEAM_SYNC"
#endif
         "]"
#endif
#if defined(TFHE_FFT_TRACK_ERROR)
         " [probe build: fp64-fft rounding margin tracked]"
#endif
#if defined(TFHE_DEV_CFG2_ONLY) || defined(TFHE_DEV_FIELD_FP_ONLY) || defined(TFHE_DEV_FIELD_FP49_ONLY) || defined(TFHE_DEV_FIELD_FFT_ONLY)
         " [subset build: not every shape / backend]"
#endif
      ;
}

const char* tfhe_status_string(int status) {
  switch (status) {
    case TFHE_OK: return "ok";
    case TFHE_ERR_INVALID_PARAMS: return "invalid parameter set";
    case TFHE_ERR_UNSUPPORTED: return "unsupported shape";
    case TFHE_ERR_NO_KEY: return "bootstrapping key not loaded";
    case TFHE_ERR_HIP: return "HIP runtime error";
    case TFHE_ERR_INVALID_ARGUMENT: return "invalid argument";
    case TFHE_ERR_NO_DEVICE: return "no GPU device (this library has no CPU path)";
    case TFHE_ERR_EXACTNESS: return "parameter set exceeds the exact-NTT bound";
    case TFHE_ERR_IO: return "file missing, truncated, not in this format, or corrupt";
    default: return "unknown status";
  }
}

void tfhe_params_default(tfhe_params* p, int cfg_test) {
  p->glwe_dimension = 2;
  p->glwe_poly_degree = 9;
  p->lwe_dimension = cfg_test ? 4 : 722;
  p->padding_bits = 1;
  p->log_p = 2;
  p->log_q = 32;
  p->ks_decomposer = {4, 5, 32};
  p->pbs_decomposer = {4, 6, 32};
}

int tfhe_params_validate(const tfhe_params* p) {
  if (!p) return TFHE_ERR_INVALID_ARGUMENT;
  if (p->log_q != 32) return TFHE_ERR_INVALID_PARAMS;
  if (decomposer_validate(p->pbs_decomposer) || decomposer_validate(p->ks_decomposer))
    return TFHE_ERR_INVALID_PARAMS;
  if (p->glwe_poly_degree == 0 || p->glwe_poly_degree + 1 >= 32) return TFHE_ERR_INVALID_PARAMS;
  if (p->log_p + p->padding_bits > 32) return TFHE_ERR_INVALID_PARAMS;  // glwe.rs:145
  if (p->log_p > p->glwe_poly_degree) return TFHE_ERR_INVALID_PARAMS;   // test_vector.rs:46
  if (p->lwe_dimension == 0 || p->glwe_dimension == 0) return TFHE_ERR_INVALID_PARAMS;
  return TFHE_OK;
}

const char* tfhe_last_error(const tfhe_context* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int tfhe_context_create_with_backend(const tfhe_params* params, int device, int backend,
                                     tfhe_context** out) {
  if (!params || !out) return TFHE_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int st = tfhe_params_validate(params);
  if (st != TFHE_OK) return st;
  if (!launch::shape_supported(params->glwe_poly_degree, params->glwe_dimension))
    return TFHE_ERR_UNSUPPORTED;
  // exactness of the integer convolution in the chosen field
  // (the fp64 field also relies on |digit| <= B <= 2^kSmallBits for its reduction-free first stage)
  const bool fp_ok = convolution_bits(params, FpField::key_bits()) < FpField::exact_bits() &&
                     params->pbs_decomposer.log_base <= (uint32_t)FpField::kSmallBits;
  const bool fp49_ok = convolution_bits(params, Fp49Field::key_bits()) < Fp49Field::exact_bits() &&
                       (params->glwe_dimension + 1) * params->pbs_decomposer.levels <= (uint32_t)Fp49Field::kMaxRows;
  const bool gl_ok = convolution_bits(params, GlField::key_bits()) < GlField::exact_bits();
  const bool gls_ok = convolution_bits(params, GlSplitField::key_bits()) < GlSplitField::exact_bits();
  // the complex transform is exact while the proven rounding error of an output coefficient stays below
  // FftField::kMaxError (field_fft.h)
  const bool fft_ok = launch::field_shape_supported(launch::kFieldFft, params->glwe_poly_degree) &&
                      params->pbs_decomposer.log_base <= (uint32_t)FftField::kMaxLogBase &&
                      FftField::error_bound((int)params->glwe_poly_degree,
                                            (int)((params->glwe_dimension + 1) * params->pbs_decomposer.levels),
                                            (int)params->pbs_decomposer.log_base) < FftField::kMaxError;
  int field = 0;
  if (backend == TFHE_BACKEND_AUTO) {
    const char* env = std::getenv("TFHE_HIP_BACKEND");
    if (env && std::strcmp(env, "goldilocks") == 0) backend = TFHE_BACKEND_GOLDILOCKS;
    else if (env && std::strcmp(env, "fp64") == 0) backend = TFHE_BACKEND_FP64;
    else if (env && std::strcmp(env, "fp64-p49") == 0) backend = TFHE_BACKEND_FP64_P49;
    else if (env && std::strcmp(env, "goldilocks-split") == 0) backend = TFHE_BACKEND_GOLDILOCKS_SPLIT;
    else if (env && std::strcmp(env, "fp64-fft") == 0) backend = TFHE_BACKEND_FP64_FFT;
  }
  // AUTO: the complex transform wherever its rounding bound holds.  (Round 2 kept the single-spectrum 49-bit field for
  // products of more than 8 digit rows, where fp64-fft's two spectra per key polynomial made the key stream decide.
  // Since round 3 -- six-FMA butterflies, twiddles fetched a transpose ahead, two samples per team at N = 512 with
  // k = 2 and at N = 2048 -- it is ahead or level there too, blind rotation of 2048 samples, profiles/r03_auto_choice.txt:
  // the reference's default parameters (18 rows) 37.5 against 40.8 ms; N = 1024, k = 1, l = 10 (20 rows) 58.2 against
  // 65.3; N = 512, k = 1, l = 6 (12 rows) 19.8 against 20.0; N = 2048, k = 2, l = 5 (15 rows, 512 samples) 34.3 against 34.2.)
  if (backend == TFHE_BACKEND_AUTO)
    field = fft_ok ? launch::kFieldFft
            : fp49_ok ? launch::kFieldFp49
            : fp_ok ? launch::kFieldFp64
            : gl_ok ? launch::kFieldGoldilocks
                    : launch::kFieldGoldilocksSplit;
  else if (backend == TFHE_BACKEND_GOLDILOCKS) field = launch::kFieldGoldilocks;
  else if (backend == TFHE_BACKEND_FP64) field = launch::kFieldFp64;
  else if (backend == TFHE_BACKEND_GOLDILOCKS_SPLIT) field = launch::kFieldGoldilocksSplit;
  else if (backend == TFHE_BACKEND_FP64_P49) field = launch::kFieldFp49;
  else if (backend == TFHE_BACKEND_FP64_FFT) field = launch::kFieldFft;
  else return TFHE_ERR_INVALID_ARGUMENT;
  if (field == launch::kFieldFft && !launch::field_shape_supported(field, params->glwe_poly_degree)) return TFHE_ERR_UNSUPPORTED;
  if ((field == launch::kFieldFft && !fft_ok) || (field == launch::kFieldFp49 && !fp49_ok) || (field == launch::kFieldFp64 && !fp_ok) || (field == launch::kFieldGoldilocks && !gl_ok) ||
      (field == launch::kFieldGoldilocksSplit && !gls_ok))
    return TFHE_ERR_EXACTNESS;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return TFHE_ERR_NO_DEVICE;

  tfhe_context* ctx = new (std::nothrow) tfhe_context();
  if (!ctx) return TFHE_ERR_HIP;
  ctx->params = *params;
  ctx->device = device;
  ctx->field = field;
  ctx->parts = launch::field_parts(field);
  ctx->N = 1u << params->glwe_poly_degree;
  ctx->R = (params->glwe_dimension + 1) * params->pbs_decomposer.levels;
  ctx->big_n = ctx->N * params->glwe_dimension;  // lib.rs:60

  ctx->pbs.n = params->lwe_dimension;
  ctx->pbs.k = params->glwe_dimension;
  ctx->pbs.log_n = params->glwe_poly_degree;
  ctx->pbs.tv_shift = 32 - params->log_p - params->padding_bits;
  ctx->pbs.log_base = params->pbs_decomposer.log_base;
  ctx->pbs.levels = params->pbs_decomposer.levels;
  ctx->pbs.ignored_bits = 32 - ctx->pbs.log_base * ctx->pbs.levels;
  ctx->pbs.first_shift = gadget_top(ctx, ctx->pbs.log_base) - ctx->pbs.log_base * ctx->pbs.levels;
  ctx->ks.log_base = params->ks_decomposer.log_base;
  ctx->ks.levels = params->ks_decomposer.levels;
  ctx->ks.ignored_bits = 32 - ctx->ks.log_base * ctx->ks.levels;
  ctx->ks.first_shift = gadget_top(ctx, ctx->ks.log_base) - ctx->ks.log_base * ctx->ks.levels;

  auto bail = [&](hipError_t e, const char* what) {
    std::fprintf(stderr, "tfhe_context_create: %s: %s\n", what, hipGetErrorString(e));
    tfhe_context_destroy(ctx);
    return TFHE_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
  if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess)
    return bail(e, "hipStreamCreate");
  ctx->own_stream = true;
  if ((e = hipStreamCreateWithFlags(&ctx->side.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&ctx->side.fork, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&ctx->side.join, hipEventDisableTiming)) != hipSuccess)
    return bail(e, "side stream");
  for (auto& slot : ctx->ev_ring)
    for (auto& ev : slot)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e, "hipEventCreate");
  st = field == launch::kFieldFp64   ? upload_twiddles<FpField>(ctx)
       : field == launch::kFieldFp49 ? upload_twiddles<Fp49Field>(ctx)
       : field == launch::kFieldFft  ? upload_twiddles<FftField>(ctx)
                                     : upload_twiddles<GlField>(ctx);  // both Goldilocks fields share the table
  if (st == TFHE_OK) st = upload_block_roots(ctx);
  if (st == TFHE_OK) st = ctx->d_queue.grow(ctx, 2 * sizeof(unsigned long long));
  if (st != TFHE_OK) {
    std::fprintf(stderr, "tfhe_context_create: twiddles / work queue: %s\n", ctx->last_error.c_str());
    tfhe_context_destroy(ctx);
    return TFHE_ERR_HIP;
  }
  if ((e = hipMemset(ctx->d_queue.as(), 0, 2 * sizeof(unsigned long long))) != hipSuccess) return bail(e, "work queue");
  // TFHE_KERNEL_SHAPE=wide|team: the starting value of tfhe_context_set_kernel_shape (test sweeps: the whole suite under
  // one shape); unset or anything else: TFHE_SHAPE_AUTO
  if (const char* shape = std::getenv("TFHE_KERNEL_SHAPE")) {
    if (std::strcmp(shape, "wide") == 0) ctx->shape = TFHE_SHAPE_WIDE;
    else if (std::strcmp(shape, "team") == 0) ctx->shape = TFHE_SHAPE_TEAM;
  }
  *out = ctx;
  return TFHE_OK;
}

int tfhe_context_create(const tfhe_params* params, int device, tfhe_context** out) {
  return tfhe_context_create_with_backend(params, device, TFHE_BACKEND_AUTO, out);
}

const char* tfhe_context_backend(const tfhe_context* ctx) {
  if (!ctx) return "";
  return ctx->field == launch::kFieldFp64     ? "fp64-p42"
         : ctx->field == launch::kFieldFp49   ? "fp64-p49"
         : ctx->field == launch::kFieldFft    ? "fp64-fft"
         : ctx->field == launch::kFieldGoldilocks ? "goldilocks"
                                                  : "goldilocks-split";
}

int tfhe_prepared_ggsw_words(const tfhe_context* ctx, size_t* words) {
  if (!ctx || !words) return TFHE_ERR_INVALID_ARGUMENT;
  *words = prepared_ggsw_words(ctx);
  return TFHE_OK;
}

void tfhe_context_destroy(tfhe_context* ctx) {
  if (!ctx) return;
  // the device is selected and both streams are drained before `delete` releases the context's device buffers
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& slot : ctx->ev_ring)
    for (auto& ev : slot)
    if (ev) (void)hipEventDestroy(ev);
  if (ctx->side.stream) {
    (void)hipStreamSynchronize(ctx->side.stream);
    (void)hipStreamDestroy(ctx->side.stream);
  }
  if (ctx->side.fork) (void)hipEventDestroy(ctx->side.fork);
  if (ctx->side.join) (void)hipEventDestroy(ctx->side.join);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int tfhe_context_set_stream(tfhe_context* ctx, void* hip_stream) {
  TFHE_TRY(check_ctx(ctx));
  if (ctx->stream || !ctx->own_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->own_stream && ctx->stream) HIP_TRY(ctx, hipStreamDestroy(ctx->stream));
  // a null handle is HIP's default stream, which is what torch.cuda.current_stream().cuda_stream
  // is unless the caller switched streams
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  ctx->own_stream = false;
  return TFHE_OK;
}

int tfhe_context_use_own_stream(tfhe_context* ctx) {
  TFHE_TRY(check_ctx(ctx));
  if (ctx->own_stream) return TFHE_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  ctx->own_stream = true;
  return TFHE_OK;
}

int tfhe_context_set_decomposer_alignment(tfhe_context* ctx, int aligned) {
  TFHE_TRY(check_ctx(ctx));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->aligned = aligned != 0;
  ctx->pbs.first_shift = gadget_top(ctx, ctx->pbs.log_base) - ctx->pbs.log_base * ctx->pbs.levels;
  ctx->ks.first_shift = gadget_top(ctx, ctx->ks.log_base) - ctx->ks.log_base * ctx->ks.levels;
  return TFHE_OK;
}

int tfhe_context_set_kernel_shape(tfhe_context* ctx, int shape) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  if (shape != TFHE_SHAPE_AUTO && shape != TFHE_SHAPE_WIDE && shape != TFHE_SHAPE_TEAM)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "kernel shape: TFHE_SHAPE_AUTO, TFHE_SHAPE_WIDE or TFHE_SHAPE_TEAM");
  ctx->shape = shape;
  return TFHE_OK;
}

int tfhe_context_set_key_switch_path(tfhe_context* ctx, int path) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  if (path != TFHE_KS_PATH_AUTO && path != TFHE_KS_PATH_SCALAR && path != TFHE_KS_PATH_MATRIX)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "key-switch path: TFHE_KS_PATH_AUTO, TFHE_KS_PATH_SCALAR or TFHE_KS_PATH_MATRIX");
  if (path == TFHE_KS_PATH_MATRIX && !ks_matrix_admitted(ctx))
    return fail(ctx, TFHE_ERR_UNSUPPORTED,
                "the matrix-core key switch needs key-switch digits that fit int8 (log_base <= 6) and int32 plane sums "
                "that cannot overflow (k N levels 2^(log_base + 7) < 2^31): this parameter set runs the scalar kernel");
  ctx->ks_path = path;
  return TFHE_OK;
}

int tfhe_debug_key_switch_plan(tfhe_context* ctx, size_t batch, int* path, unsigned* grid_x, unsigned* grid_y,
                               unsigned* splits) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {path, grid_x, grid_y, splits}, 1, "null pointer"));
  if (batch == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch == 0");
  launch::KeySwitchPlanInfo plan{};
  HIP_TRY(ctx, launch::key_switch_plan(ctx->ks, ctx->big_n, ctx->params.lwe_dimension, batch, ctx->ks_path, &plan));
  *path = plan.matrix ? TFHE_KS_PATH_MATRIX : TFHE_KS_PATH_SCALAR;
  *grid_x = plan.grid_x;
  *grid_y = plan.grid_y;
  *splits = plan.splits;
  return TFHE_OK;
}

int tfhe_context_set_bootstrap_order(tfhe_context* ctx, int ks_first) {
  TFHE_TRY(check_ctx(ctx));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->ks_first = ks_first != 0;
  return TFHE_OK;
}

int tfhe_context_synchronize(tfhe_context* ctx) {
  TFHE_TRY(check_ctx(ctx));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_OK;
}

int tfhe_context_reserve(tfhe_context* ctx, size_t max_batch) {
  TFHE_TRY(check_ctx(ctx));
  if (max_batch == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_batch == 0");
  return reserve(ctx, max_batch);
}

int tfhe_context_set_timing(tfhe_context* ctx, int enable) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  ctx->timing = enable != 0;
  ctx->ev_valid_br = ctx->ev_valid_ks = ctx->ev_valid_mb = false;
  ctx->timed_bootstraps = 0;
  return TFHE_OK;
}

int tfhe_measure_hbm_copy(tfhe_context* ctx, size_t bytes, int reps, double* gb_per_s) {
  TFHE_TRY(check_ctx(ctx));
  if (!gb_per_s || bytes < 16 || reps <= 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "bytes >= 16, reps >= 1");
  bytes &= ~(size_t)15;
  DeviceBuffer src_buf, dst_buf;
  TFHE_TRY(src_buf.grow(ctx, bytes));
  TFHE_TRY(dst_buf.grow(ctx, bytes));
  void *src = src_buf.as(), *dst = dst_buf.as();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipMemsetAsync(src, 1, bytes, ctx->stream);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = launch::stream_copy(ctx->stream, src, dst, bytes);
  if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
  for (int i = 0; i < reps && e == hipSuccess; ++i) e = launch::stream_copy(ctx->stream, src, dst, bytes);
  if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (e != hipSuccess) return hip_fail(ctx, e, "hbm copy probe");
  *gb_per_s = 2.0 * (double)bytes * reps / ((double)ms * 1e-3) / 1e9;  // read + write
  return TFHE_OK;
}

int tfhe_debug_fft_margin(tfhe_context* ctx, double* worst, int reset) {
  TFHE_TRY(check_ctx(ctx));
#if defined(TFHE_FFT_TRACK_ERROR)
  HIP_TRY(ctx, launch::fft_margin(worst, reset != 0));
  return TFHE_OK;
#else
  (void)worst;
  (void)reset;
  return fail(ctx, TFHE_ERR_UNSUPPORTED, "this build carries no rounding-margin probe (libtfhe_hip_probe.so does)");
#endif
}

int tfhe_debug_blind_rotate_plan(tfhe_context* ctx, size_t batch, size_t* samples_per_group, unsigned* segments,
                                 unsigned* streams, size_t* resident_samples) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {samples_per_group, segments, streams, resident_samples}, 1, "null pointer"));
  launch::BlindRotatePlanInfo plan{};
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the plan of tfhe_bootstrap_batch[_device], which reserve the workspace the accumulators are parked in
  HIP_TRY(ctx, launch::blind_rotate_plan(ctx->field, ctx->pbs, batch, !ctx->bmmp, ctx->side.stream != nullptr, &plan, ctx->shape));
  *samples_per_group = plan.chunk;
  *segments = ctx->bmmp ? 1u : plan.segments;
  *streams = ctx->bmmp ? 1u : (unsigned)plan.streams;
  *resident_samples = plan.resident_samples;
  return TFHE_OK;
}

int tfhe_debug_blind_rotate_shape(tfhe_context* ctx, size_t batch, unsigned* waves_per_sample, unsigned* samples_per_team) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {waves_per_sample, samples_per_team}, 1, "null pointer"));
  launch::BlindRotatePlanInfo plan{};
  HIP_TRY(ctx, launch::blind_rotate_plan(ctx->field, ctx->pbs, batch, !ctx->bmmp, ctx->side.stream != nullptr, &plan, ctx->shape));
  *waves_per_sample = (unsigned)plan.waves_per_sample;
  *samples_per_team = (unsigned)plan.samples_per_team;
  return TFHE_OK;
}

int tfhe_kernel_ms_ago(tfhe_context* ctx, unsigned steps_ago, float* blind_rotate_ms, float* key_switch_ms) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {blind_rotate_ms, key_switch_ms}, 1, "null pointer"));
  if (steps_ago >= (unsigned)tfhe_context::kTimingSlots || (unsigned long long)steps_ago >= ctx->timed_bootstraps)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "no timed bootstrap that far back");
  hipEvent_t* ev = ctx->ev_ring[(ctx->ev_slot + tfhe_context::kTimingSlots - (int)steps_ago) % tfhe_context::kTimingSlots];
  HIP_TRY(ctx, hipEventSynchronize(ev[1]));
  HIP_TRY(ctx, hipEventElapsedTime(blind_rotate_ms, ev[0], ev[1]));
  HIP_TRY(ctx, hipEventSynchronize(ev[3]));
  HIP_TRY(ctx, hipEventElapsedTime(key_switch_ms, ev[2], ev[3]));
  return TFHE_OK;
}

int tfhe_last_kernel_ms(tfhe_context* ctx, float* blind_rotate_ms, float* key_switch_ms) {
  TFHE_TRY(check_ctx(ctx));
  if (blind_rotate_ms) *blind_rotate_ms = -1.0f;
  if (key_switch_ms) *key_switch_ms = -1.0f;
  if (ctx->ev_valid_br && blind_rotate_ms) {
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(blind_rotate_ms, ctx->ev[0], ctx->ev[1]));
  }
  if (ctx->ev_valid_ks && key_switch_ms) {
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[3]));
    HIP_TRY(ctx, hipEventElapsedTime(key_switch_ms, ctx->ev[2], ctx->ev[3]));
  }
  return TFHE_OK;
}

// ---------------------------------------------------------------------------------- keys
// GGSWs of a bootstrapping key: one per key bit, or three per pair of key bits (BMMP)
static size_t key_ggsws(const tfhe_context* ctx, bool bmmp) {
  const size_t n = ctx->params.lwe_dimension;
  return bmmp ? n / 2 * 3 : n;
}

static int check_bmmp(tfhe_context* ctx) {
  if (!launch::shape_supported_bmmp(ctx->pbs.log_n, ctx->pbs.k) || (ctx->params.lwe_dimension & 1u))
    return fail(ctx, TFHE_ERR_UNSUPPORTED, "the unrolled (BMMP) blind rotation needs N = 512 and an even lwe_dimension");
  if (!launch::field_supported_bmmp(ctx->field))
    return fail(ctx, TFHE_ERR_UNSUPPORTED,
                std::string("the unrolled (BMMP) blind rotation is offered in the goldilocks and fp64-p49 backends only (its three "
                            "accumulator sets spill 50-172 registers in the others and it runs slower than the loop there); this "
                            "context uses ") + tfhe_context_backend(ctx) + ": create it with TFHE_BACKEND_GOLDILOCKS or "
                            "TFHE_BACKEND_FP64_P49, or load an ordinary key");
  return TFHE_OK;
}

static int load_key_common(tfhe_context* ctx, const u32* d_bsk_raw, const u32* d_ksk_raw,
                           bool ksk_needs_copy, bool bmmp = false) {
  const size_t ggsws = key_ggsws(ctx, bmmp);
  const size_t bsk_polys = ggsws * ctx->R * (ctx->params.glwe_dimension + 1);
  // the key buffers are overwritten in place: until the new key is complete the context holds none (a failure half way
  // must not leave it bootstrapping under a half-written key)
  ctx->have_key = false;
  TFHE_TRY(ensure_key_buffers(ctx, ggsws, ks_matrix_admitted(ctx)));
  HIP_TRY(ctx, launch::bsk_prepare(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->pbs.k, ctx->d_tw.as(), d_bsk_raw, bsk_polys, ctx->d_bsk.as()));
  if (ksk_needs_copy)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ksk.as<u32>(), d_ksk_raw, ksk_words(ctx) * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
  // the key-switching key's byte planes for the matrix cores, made once per key like the BSK's spectra
  if (ks_matrix_admitted(ctx)) {
    HIP_TRY(ctx, launch::ksk_prepare_matrix(ctx->stream, ctx->ks, ctx->big_n, ctx->params.lwe_dimension, ctx->d_ksk.as<u32>(),
                                            ctx->d_ksk_matrix.as()));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->have_key = true;
  ctx->bmmp = bmmp;
  return TFHE_OK;
}

static int load_key_host(tfhe_context* ctx, const uint32_t* bsk, const uint32_t* ksk, bool bmmp) {
  if (!bsk || !ksk) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null key pointer");
  const size_t bsk_words = key_ggsws(ctx, bmmp) * ggsw_words(ctx);
  DeviceBuffer raw;
  TFHE_TRY(raw.grow(ctx, bsk_words * sizeof(u32)));
  HIP_TRY(ctx, hipMemcpy(raw.as(), bsk, bsk_words * sizeof(u32), hipMemcpyHostToDevice));
  // The key-switching key's buffer alone, absent only before a context's first key: the context still answers under
  // the key it holds, so the prepared BSK is not touched here (ensure_key_buffers, in load_key_common, resizes it once
  // that key is out of service).
  TFHE_TRY(ctx->d_ksk.grow(ctx, ksk_words(ctx) * sizeof(u32)));
  // the key-switching key is overwritten in place by a copy that does not order itself behind the context's stream:
  // whatever was enqueued under the old key finishes first, and from here on the context holds no key
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->have_key = false;
  HIP_TRY(ctx, hipMemcpy(ctx->d_ksk.as<u32>(), ksk, ksk_words(ctx) * sizeof(u32), hipMemcpyHostToDevice));
  return load_key_common(ctx, raw.as<u32>(), nullptr, false, bmmp);
}

int tfhe_load_bootstrapping_key(tfhe_context* ctx, const uint32_t* bsk, const uint32_t* ksk) {
  TFHE_TRY(check_ctx(ctx));
  return load_key_host(ctx, bsk, ksk, false);
}

int tfhe_load_bootstrapping_key_device(tfhe_context* ctx, const uint32_t* bsk, const uint32_t* ksk) {
  TFHE_TRY(check_ctx(ctx));
  if (!bsk || !ksk) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null key pointer");
  return load_key_common(ctx, bsk, ksk, true);
}

int tfhe_load_bootstrapping_key_bmmp(tfhe_context* ctx, const uint32_t* bsk_bmmp, const uint32_t* ksk) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_bmmp(ctx));
  return load_key_host(ctx, bsk_bmmp, ksk, true);
}

int tfhe_load_bootstrapping_key_bmmp_device(tfhe_context* ctx, const uint32_t* bsk_bmmp, const uint32_t* ksk) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_bmmp(ctx));
  if (!bsk_bmmp || !ksk) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null key pointer");
  return load_key_common(ctx, bsk_bmmp, ksk, true, true);
}

int tfhe_context_uses_bmmp(const tfhe_context* ctx) { return ctx && ctx->have_key && ctx->bmmp ? 1 : 0; }

// ---------------------------------------------------------------------------------- bootstrap
namespace {
// The arguments of a rotation or a bootstrap, clear test vectors or (rotation_offset given) GLWE accumulators [count]
int check_rotate_args(tfhe_context* ctx, const void* lwe_in, const void* acc, const void* out, size_t batch, size_t count,
                      const size_t* rotation_offset = nullptr) {
  TFHE_TRY(check_batch(ctx, {lwe_in, acc, out}, batch, count, rotation_offset ? "acc_count" : "tv_count"));
  if (rotation_offset && *rotation_offset >= 2 * (size_t)ctx->N)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "rotation_offset must be below 2N = " + std::to_string(2 * (size_t)ctx->N));
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "load the bootstrapping key first");
  if (rotation_offset && ctx->bmmp)
    return fail(ctx, TFHE_ERR_UNSUPPORTED,
                "a BMMP key is loaded: the unrolled rotation starts from a clear test vector only (load a plain "
                "bootstrapping key for a GLWE accumulator)");
  return TFHE_OK;
}

// rotation only, timed as one
int rotate_device(tfhe_context* ctx, const u32* lwe_in, size_t batch, const u32* acc, size_t count, u32* glwe_out, AccSource from) {
  TFHE_TRY(span_begin(ctx, kRotationSpan));
  HIP_TRY(ctx, enqueue_blind_rotate(ctx, lwe_in, batch, acc, count, glwe_out, nullptr, from));
  return span_end(ctx, kRotationSpan);
}
}  // namespace

int tfhe_bootstrap_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch,
                                const uint32_t* tv, size_t tv_count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, tv, lwe_out, batch, tv_count));
  TFHE_TRY(reserve(ctx, batch));
  return enqueue_bootstrap(ctx, lwe_in, batch, tv, tv_count, ctx->d_lwe_big.as<u32>(), lwe_out);
}

int tfhe_bootstrap_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, const uint32_t* tv,
                         size_t tv_count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, tv, lwe_out, batch, tv_count));
  TFHE_TRY(check_tv_host(ctx, tv, tv_count * ctx->N));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * io_words(ctx)));
  TFHE_TRY(upload(ctx, ctx->d_tv.as<u32>(), tv, tv_count * ctx->N));
  TFHE_TRY(enqueue_bootstrap(ctx, ctx->d_lwe_in.as<u32>(), batch, ctx->d_tv.as<u32>(), tv_count, ctx->d_lwe_big.as<u32>(), ctx->d_lwe_out.as<u32>()));
  return download_and_wait(ctx, lwe_out, ctx->d_lwe_out.as<u32>(), batch * io_words(ctx));
}

int tfhe_blind_rotate_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch,
                                   const uint32_t* tv, size_t tv_count, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, tv, glwe_out, batch, tv_count));
  return rotate_device(ctx, lwe_in, batch, tv, tv_count, glwe_out, AccSource());
}

// (the rotation-only forms read n+1 words per input whatever the bootstrap order is)
int tfhe_blind_rotate_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch,
                            const uint32_t* tv, size_t tv_count, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, tv, glwe_out, batch, tv_count));
  TFHE_TRY(check_tv_host(ctx, tv, tv_count * ctx->N));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * lwe_words(ctx)));
  TFHE_TRY(upload(ctx, ctx->d_tv.as<u32>(), tv, tv_count * ctx->N));
  TFHE_TRY(rotate_device(ctx, ctx->d_lwe_in.as<u32>(), batch, ctx->d_tv.as<u32>(), tv_count, ctx->d_glwe_a.as<u32>(), AccSource()));
  return download_and_wait(ctx, glwe_out, ctx->d_glwe_a.as<u32>(), batch * glwe_words(ctx));
}

// ------------------------------------------------- blind rotation / bootstrap from a GLWE accumulator
int tfhe_blind_rotate_glwe_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, const uint32_t* acc_in,
                                        size_t acc_count, size_t rotation_offset, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, acc_in, glwe_out, batch, acc_count, &rotation_offset));
  return rotate_device(ctx, lwe_in, batch, acc_in, acc_count, glwe_out, AccSource{true, (u32)rotation_offset});
}

int tfhe_blind_rotate_glwe_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, const uint32_t* acc_in,
                                 size_t acc_count, size_t rotation_offset, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, acc_in, glwe_out, batch, acc_count, &rotation_offset));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * lwe_words(ctx)));
  TFHE_TRY(upload(ctx, ctx->d_glwe_a.as<u32>(), acc_in, acc_count * glwe_words(ctx)));
  TFHE_TRY(rotate_device(ctx, ctx->d_lwe_in.as<u32>(), batch, ctx->d_glwe_a.as<u32>(), acc_count, ctx->d_glwe_b.as<u32>(), AccSource{true, (u32)rotation_offset}));
  return download_and_wait(ctx, glwe_out, ctx->d_glwe_b.as<u32>(), batch * glwe_words(ctx));
}

int tfhe_bootstrap_glwe_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, const uint32_t* acc_in,
                                     size_t acc_count, size_t rotation_offset, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, acc_in, lwe_out, batch, acc_count, &rotation_offset));
  TFHE_TRY(reserve(ctx, batch));
  return enqueue_bootstrap(ctx, lwe_in, batch, acc_in, acc_count, ctx->d_lwe_big.as<u32>(), lwe_out, AccSource{true, (u32)rotation_offset});
}

int tfhe_bootstrap_glwe_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, const uint32_t* acc_in,
                              size_t acc_count, size_t rotation_offset, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_rotate_args(ctx, lwe_in, acc_in, lwe_out, batch, acc_count, &rotation_offset));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * io_words(ctx)));
  TFHE_TRY(upload(ctx, ctx->d_glwe_a.as<u32>(), acc_in, acc_count * glwe_words(ctx)));
  TFHE_TRY(enqueue_bootstrap(ctx, ctx->d_lwe_in.as<u32>(), batch, ctx->d_glwe_a.as<u32>(), acc_count, ctx->d_lwe_big.as<u32>(), ctx->d_lwe_out.as<u32>(),
                             AccSource{true, (u32)rotation_offset}));
  return download_and_wait(ctx, lwe_out, ctx->d_lwe_out.as<u32>(), batch * io_words(ctx));
}

int tfhe_sample_extract_batch(tfhe_context* ctx, const uint32_t* glwe, size_t batch,
                              size_t sample_index, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe, lwe_out}, batch));
  if (sample_index >= ctx->N)  // assert!(sample_index < degree), bootstrapping.rs:127
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "sample_index >= N (bootstrapping.rs:127)");
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_glwe_a.as<u32>(), glwe, batch * glwe_words(ctx)));
  HIP_TRY(ctx, launch::sample_extract(ctx->stream, ctx->pbs.log_n, ctx->pbs.k, ctx->d_glwe_a.as<u32>(), batch,
                                      (u32)sample_index, ctx->d_lwe_big.as<u32>()));
  return download_and_wait(ctx, lwe_out, ctx->d_lwe_big.as<u32>(), batch * big_lwe_words(ctx));
}

namespace {
int check_key_switch_args(tfhe_context* ctx, const void* lwe_in, const void* lwe_out, size_t batch) {
  TFHE_TRY(check_present(ctx, {lwe_in, lwe_out}, batch));
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "load the bootstrapping key first");
  return TFHE_OK;
}
}  // namespace

int tfhe_key_switch_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch,
                                 uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_key_switch_args(ctx, lwe_in, lwe_out, batch));
  TFHE_TRY(span_begin(ctx, kKeySwitchSpan));
  HIP_TRY(ctx, launch::key_switch(ctx->stream, ctx->ks, ctx->big_n, ctx->params.lwe_dimension, lwe_in,
                                  batch, ctx->d_ksk.as<u32>(), lwe_out, ctx->d_ksk_matrix.as(), ctx->ks_path));
  return span_end(ctx, kKeySwitchSpan);
}

int tfhe_key_switch_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_key_switch_args(ctx, lwe_in, lwe_out, batch));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_lwe_big.as<u32>(), lwe_in, batch * big_lwe_words(ctx)));
  TFHE_TRY(tfhe_key_switch_batch_device(ctx, ctx->d_lwe_big.as<u32>(), batch, ctx->d_lwe_out.as<u32>()));
  return download_and_wait(ctx, lwe_out, ctx->d_lwe_out.as<u32>(), batch * lwe_words(ctx));
}

// ---------------------------------------------------------------------------------- ggsw.rs
int tfhe_prepare_ggsw_device(tfhe_context* ctx, const uint32_t* ggsw, size_t ggsw_count,
                             void* ggsw_prepared) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {ggsw, ggsw_prepared}, ggsw_count, "null pointer / zero count"));
  const size_t polys = ggsw_count * ctx->R * (ctx->params.glwe_dimension + 1);
  HIP_TRY(ctx, launch::bsk_prepare(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->pbs.k, ctx->d_tw.as(), ggsw, polys, ggsw_prepared));
  return TFHE_OK;
}

int tfhe_external_product_prepared_device(tfhe_context* ctx, const void* ggsw_prepared,
                                          size_t ggsw_count, const uint32_t* glwe_in, size_t batch,
                                          uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_batch(ctx, {ggsw_prepared, glwe_in, glwe_out}, batch, ggsw_count, "ggsw_count", kProducts));
  TFHE_TRY(span_begin(ctx, kRotationSpan));
  HIP_TRY(ctx, launch::external_product(ctx->stream, ctx->field, ctx->pbs, ctx->d_tw.as(), ggsw_prepared,
                                        ggsw_count == 1 ? 0 : prepared_ggsw_words(ctx), glwe_in,
                                        nullptr, nullptr, batch, glwe_out, ctx->d_queue.as<unsigned long long>()));
  return span_end(ctx, kRotationSpan);
}

// host GGSWs: uploaded raw, prepared into d_ggsw_tmp
static int upload_and_prepare_ggsw(tfhe_context* ctx, const u32* ggsw, size_t ggsw_count) {
  const size_t words = ggsw_count * ggsw_words(ctx);
  TFHE_TRY(ctx->d_ggsw_raw.grow(ctx, words * sizeof(u32)));
  TFHE_TRY(ctx->d_ggsw_tmp.grow(ctx, words * ctx->parts * sizeof(u64)));
  TFHE_TRY(upload(ctx, ctx->d_ggsw_raw.as<u32>(), ggsw, words));
  return tfhe_prepare_ggsw_device(ctx, ctx->d_ggsw_raw.as<u32>(), ggsw_count, ctx->d_ggsw_tmp.as());
}

int tfhe_external_product_batch(tfhe_context* ctx, const uint32_t* ggsw, size_t ggsw_count,
                                const uint32_t* glwe_in, size_t batch, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_batch(ctx, {ggsw, glwe_in, glwe_out}, batch, ggsw_count, "ggsw_count", kHostProducts));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload_and_prepare_ggsw(ctx, ggsw, ggsw_count));
  TFHE_TRY(upload(ctx, ctx->d_glwe_a.as<u32>(), glwe_in, batch * glwe_words(ctx)));
  TFHE_TRY(tfhe_external_product_prepared_device(ctx, ctx->d_ggsw_tmp.as(), ggsw_count,
                                                 ctx->d_glwe_a.as<u32>(), batch, ctx->d_glwe_b.as<u32>()));
  return download_and_wait(ctx, glwe_out, ctx->d_glwe_b.as<u32>(), batch * glwe_words(ctx));
}

int tfhe_cmux_batch(tfhe_context* ctx, const uint32_t* ggsw, size_t ggsw_count, const uint32_t* ct0,
                    uint32_t* ct1, size_t batch, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_batch(ctx, {ggsw, ct0, ct1, glwe_out}, batch, ggsw_count, "ggsw_count", kHostProducts));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload_and_prepare_ggsw(ctx, ggsw, ggsw_count));
  const size_t words = batch * glwe_words(ctx);
  TFHE_TRY(upload(ctx, ctx->d_glwe_a.as<u32>(), ct0, words));
  TFHE_TRY(upload(ctx, ctx->d_glwe_b.as<u32>(), ct1, words));
  HIP_TRY(ctx, launch::external_product(ctx->stream, ctx->field, ctx->pbs, ctx->d_tw.as(), ctx->d_ggsw_tmp.as(),
                                        ggsw_count == 1 ? 0 : prepared_ggsw_words(ctx), nullptr,
                                        ctx->d_glwe_b.as<u32>(), ctx->d_glwe_a.as<u32>(), batch, ctx->d_glwe_c.as<u32>(), ctx->d_queue.as<unsigned long long>()));
  TFHE_TRY(download(ctx, glwe_out, ctx->d_glwe_c.as<u32>(), words));
  return download_and_wait(ctx, ct1, ctx->d_glwe_b.as<u32>(), words);
}

// ---------------------------------------------------------------------------------- CMUX tree / table lookup
// include/tfhe_hip.h states the operations, pbs_wave.h::cmux_tree_team the walk, passes.h the plan and the passes.
namespace {

constexpr size_t kMaxTreeDepth = 20;

// the plan of a tree of the lookup (cmux_tree_kernel's residency, the lookup's forced height) or of the update
int tree_plan_of(tfhe_context* ctx, bool demux, size_t trees, size_t depth, passes::TreePlan* plan) {
  unsigned resident = 0;
  hipError_t e = demux ? launch::demux_resident_teams(ctx->field, ctx->pbs, &resident)
                       : launch::tree_resident_teams(ctx->field, ctx->pbs, &resident);
  if (e == hipSuccess && !passes::lookup_plan_for(trees, (u32)depth, demux ? ctx->demux_height : ctx->lookup_height, resident,
                                                  glwe_words(ctx), plan))
    e = hipErrorInvalidValue;
  if (e == hipErrorInvalidValue)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "trees * 2^(depth - subtree height) exceeds the 2^31 - 1 teams of one launch");
  if (e != hipSuccess) return hip_fail(ctx, e, demux ? "demux plan" : "lookup plan");
  return TFHE_OK;
}

int grow_lookup_workspace(tfhe_context* ctx, size_t words) { return ctx->d_lookup_ws.grow(ctx, words * sizeof(u32)); }

// What a tree / lookup call reads its leaves from: GLWEs [sets][tables][2^depth][k+1][N] or a clear table
// [sets][tables][2^address_bits]
struct LookupLeaves {
  const u32* glwe;
  const u32* table;
  bool shared;  // one set for all queries
};

// `tree_depth` tree levels with selectors [first, first + tree_depth) of every query's `address_bits` selectors, then
// (lwe_out only) min(address_bits, log2 N) rotation steps with selectors [0, first) and the sample extraction
int run_lookup(tfhe_context* ctx, const void* selectors, size_t queries, size_t address_bits, size_t first, size_t tree_depth,
               const LookupLeaves& leaves, size_t tables, u32* glwe_out, u32* lwe_out) {
  passes::TreePlan plan{};
  TFHE_TRY(tree_plan_of(ctx, false, queries * tables, tree_depth, &plan));
  if (plan.workspace_words > ctx->d_lookup_ws.words())
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(plan.workspace_words) + " words of lookup workspace, " +
                    std::to_string(ctx->d_lookup_ws.words()) + " are reserved (tfhe_context_reserve_lookup)");
  const passes::LookupCall call{selectors, prepared_ggsw_words(ctx), glwe_words(ctx), queries, address_bits, first, tree_depth,
                                leaves.glwe, leaves.table, leaves.shared, tables, glwe_out, lwe_out};
  size_t ws_words = 0;
  return passes::lookup_passes(plan, call, ctx->d_lookup_ws.as<u32>(), &ws_words, [&](const CmuxTreePass& pass, size_t teams) {
    HIP_TRY(ctx, launch::cmux_tree_pass(ctx->stream, ctx->field, ctx->pbs, ctx->d_tw.as(), pass, teams));
    return (int)TFHE_OK;
  });
}

int check_lookup_args(tfhe_context* ctx, const void* selectors, const void* data, const void* out, size_t queries, size_t depth,
                      size_t max_depth, size_t sets, size_t tables) {
  TFHE_TRY(check_present(ctx, {selectors, data, out}, 1, "null pointer"));
  if (queries == 0 || tables == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries and tables must be at least 1");
  if (depth == 0 || depth > max_depth)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "depth must be in [1, " + std::to_string(max_depth) + "]");
  if (sets != 1 && sets != queries) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "leaf_sets / table_sets must be 1 or queries");
  if (queries > kMaxBatch || tables > kMaxBatch || queries * tables > kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries * tables exceeds 2^31 - 1");
  return TFHE_OK;
}

}  // namespace

int tfhe_context_reserve_lookup(tfhe_context* ctx, size_t max_trees, size_t max_tree_depth, size_t max_lookup_bits) {
  TFHE_TRY(check_ctx(ctx));
  if (max_trees == 0 || max_trees > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_trees must be in [1, 2^31)");
  if (max_tree_depth > kMaxTreeDepth) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_tree_depth must be in [0, 20]");
  if (max_lookup_bits > ctx->pbs.log_n + kMaxTreeDepth)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_lookup_bits must be in [0, log2 N + 20]");
  if (max_tree_depth == 0 && max_lookup_bits == 0)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_tree_depth and max_lookup_bits are both 0: nothing to reserve for");
  // a lookup of D address bits runs a tree of D - log2 N levels (none up to log2 N bits)
  const size_t lookup_depth = max_lookup_bits > ctx->pbs.log_n ? max_lookup_bits - ctx->pbs.log_n : 0;
  return grow_lookup_workspace(ctx, passes::lookup_workspace_need(max_trees, std::max(max_tree_depth, lookup_depth), glwe_words(ctx)));
}

int tfhe_context_set_lookup_subtree_height(tfhe_context* ctx, unsigned height) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  if (height > kMaxTreeDepth) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "subtree height must be in [0, 20] (0: automatic)");
  ctx->lookup_height = height;
  return TFHE_OK;
}

int tfhe_debug_lookup_plan(tfhe_context* ctx, size_t trees, size_t depth, unsigned* subtree_height, unsigned* launches) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {subtree_height, launches}, 1, "null pointer"));
  if (trees == 0 || trees > kMaxBatch || depth > kMaxTreeDepth)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "trees must be in [1, 2^31), depth in [0, 20]");
  passes::TreePlan plan{};
  TFHE_TRY(tree_plan_of(ctx, false, trees, depth, &plan));
  *subtree_height = plan.height;
  *launches = plan.launches;
  return TFHE_OK;
}

int tfhe_cmux_prepared_device(tfhe_context* ctx, const void* ggsw_prepared, size_t ggsw_count, const uint32_t* ct0,
                              const uint32_t* ct1, size_t batch, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_batch(ctx, {ggsw_prepared, ct0, ct1, glwe_out}, batch, ggsw_count, "ggsw_count", kProducts));
  // a tree of one level per sample whose two leaves live in two arrays: one team per sample, no workspace
  CmuxTreePass pass{};
  pass.selectors = pass.rot_selectors = ggsw_prepared;
  pass.query_stride = ggsw_count == 1 ? 0 : prepared_ggsw_words(ctx);
  pass.tables = 1;
  pass.height = 1;
  pass.even = ct0;
  pass.odd = ct1;
  pass.set_stride = glwe_words(ctx);
  pass.glwe_out = glwe_out;
  HIP_TRY(ctx, launch::cmux_tree_pass(ctx->stream, ctx->field, ctx->pbs, ctx->d_tw.as(), pass, batch));
  return TFHE_OK;
}

int tfhe_cmux_tree_device(tfhe_context* ctx, const void* selectors_prepared, size_t queries, size_t depth,
                          const uint32_t* leaves, size_t leaf_sets, size_t tables, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lookup_args(ctx, selectors_prepared, leaves, glwe_out, queries, depth, kMaxTreeDepth, leaf_sets, tables));
  return run_lookup(ctx, selectors_prepared, queries, depth, 0, depth, LookupLeaves{leaves, nullptr, leaf_sets == 1 && queries > 1},
                    tables, glwe_out, nullptr);
}

int tfhe_table_lookup_device(tfhe_context* ctx, const void* selectors_prepared, size_t queries, size_t depth,
                             const uint32_t* table, size_t table_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lookup_args(ctx, selectors_prepared, table, lwe_out, queries, depth, ctx->pbs.log_n + kMaxTreeDepth, table_sets, tables));
  const size_t d_lo = std::min(depth, (size_t)ctx->pbs.log_n);
  return run_lookup(ctx, selectors_prepared, queries, depth, d_lo, depth - d_lo, LookupLeaves{nullptr, table, table_sets == 1 && queries > 1},
                    tables, nullptr, lwe_out);
}

// host forms: selectors [queries][depth][R][k+1][N] raw; everything uploaded, the selectors prepared once
static int lookup_host(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t depth, const uint32_t* data,
                       size_t sets, size_t tables, bool is_table, uint32_t* out) {
  const size_t d_lo = is_table ? std::min(depth, (size_t)ctx->pbs.log_n) : 0;
  const size_t trees = queries * tables;
  passes::TreePlan plan{};
  TFHE_TRY(tree_plan_of(ctx, false, trees, depth - d_lo, &plan));
  TFHE_TRY(grow_lookup_workspace(ctx, std::max<size_t>(plan.workspace_words, 1)));
  enum { kIn, kOut };
  Staging s(ctx, {sets * tables * ((size_t)1 << depth) * (is_table ? 1 : glwe_words(ctx)),
                  trees * (is_table ? big_lwe_words(ctx) : glwe_words(ctx))});
  TFHE_TRY(s.reserve());
  TFHE_TRY(upload_and_prepare_ggsw(ctx, selectors, queries * depth));
  TFHE_TRY(s.upload(kIn, data));
  TFHE_TRY(is_table ? tfhe_table_lookup_device(ctx, ctx->d_ggsw_tmp.as(), queries, depth, s[kIn], sets, tables, s[kOut])
                    : tfhe_cmux_tree_device(ctx, ctx->d_ggsw_tmp.as(), queries, depth, s[kIn], sets, tables, s[kOut]));
  return s.download_and_wait(kOut, out);
}

int tfhe_cmux_tree(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t depth, const uint32_t* leaves,
                   size_t leaf_sets, size_t tables, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lookup_args(ctx, selectors, leaves, glwe_out, queries, depth, kMaxTreeDepth, leaf_sets, tables));
  return lookup_host(ctx, selectors, queries, depth, leaves, leaf_sets, tables, false, glwe_out);
}

int tfhe_table_lookup(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t depth, const uint32_t* table,
                      size_t table_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lookup_args(ctx, selectors, table, lwe_out, queries, depth, ctx->pbs.log_n + kMaxTreeDepth, table_sets, tables));
  return lookup_host(ctx, selectors, queries, depth, table, table_sets, tables, true, lwe_out);
}

// ---------------------------------------------------------------------------------- DEMUX tree / table update
// include/tfhe_hip.h states the operations, pbs_wave.h::demux_tree_team the walk; the plan is the lookup's walked in
// reverse (passes.h): the top pass takes what ceil(d / h) - 1 passes of h levels leave over.
namespace {

int grow_demux_workspace(tfhe_context* ctx, size_t words) { return ctx->d_demux_ws.grow(ctx, words * sizeof(u32)); }

bool overlap(const void* a, size_t a_words, const void* b, size_t b_words) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_words * sizeof(u32) && b0 < a0 + a_words * sizeof(u32);
}

// `rot_steps` rotation steps with selectors [0, rot_steps) of every query's `address_bits` selectors on roots
// [queries][values][k+1][N], then `tree_depth` tree levels with selectors [rot_steps, rot_steps + tree_depth); the
// leaves are stored to / added into leaves [sets][values][2^tree_depth][k+1][N]
int run_demux(tfhe_context* ctx, const void* selectors, size_t queries, size_t address_bits, size_t rot_steps, size_t tree_depth,
              const u32* roots, size_t values, u32* leaves, bool shared, bool accumulate) {
  const size_t trees = queries * values;
  const size_t glwe = glwe_words(ctx);
  if (overlap(roots, trees * glwe, leaves, ((shared ? values : trees) << tree_depth) * glwe))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the output overlaps the input");
  passes::TreePlan plan{};
  TFHE_TRY(tree_plan_of(ctx, true, trees, tree_depth, &plan));
  if (plan.workspace_words > ctx->d_demux_ws.words())
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(plan.workspace_words * sizeof(u32)) + " bytes of demux workspace, " +
                    std::to_string(ctx->d_demux_ws.bytes()) + " are reserved (tfhe_context_reserve_demux)");
  const passes::DemuxCall call{selectors, prepared_ggsw_words(ctx), glwe, queries, address_bits, rot_steps, tree_depth,
                               roots, values, leaves, shared, accumulate};
  size_t ws_words = 0;
  return passes::demux_passes(plan, call, ctx->d_demux_ws.as<u32>(), &ws_words, [&](const DemuxTreePass& pass, size_t teams) {
    HIP_TRY(ctx, launch::demux_tree_pass(ctx->stream, ctx->field, ctx->pbs, ctx->d_tw.as(), pass, teams));
    return (int)TFHE_OK;
  });
}

int check_demux_args(tfhe_context* ctx, const void* selectors, const void* in, const void* out, size_t queries, size_t depth,
                     size_t max_depth, size_t sets, size_t values, bool accumulate) {
  TFHE_TRY(check_lookup_args(ctx, selectors, in, out, queries, depth, max_depth, sets, values));
  if (!accumulate && sets != queries)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "accumulate = 0 stores: every query needs its own leaf set (leaf_sets == queries)");
  return TFHE_OK;
}

}  // namespace

int tfhe_context_reserve_demux(tfhe_context* ctx, size_t max_trees, size_t max_tree_depth, size_t max_write_bits) {
  TFHE_TRY(check_ctx(ctx));
  if (max_trees == 0 || max_trees > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_trees must be in [1, 2^31)");
  if (max_tree_depth > kMaxTreeDepth) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_tree_depth must be in [0, 20]");
  if (max_write_bits > ctx->pbs.log_n + kMaxTreeDepth)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_write_bits must be in [0, log2 N + 20]");
  if (max_tree_depth == 0 && max_write_bits == 0)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_tree_depth and max_write_bits are both 0: nothing to reserve for");
  // a write of D address bits runs a tree of D - log2 N levels (none up to log2 N bits); the need is the lookup's
  const size_t write_depth = max_write_bits > ctx->pbs.log_n ? max_write_bits - ctx->pbs.log_n : 0;
  return grow_demux_workspace(ctx, passes::lookup_workspace_need(max_trees, std::max(max_tree_depth, write_depth), glwe_words(ctx)));
}

int tfhe_context_set_demux_subtree_height(tfhe_context* ctx, unsigned height) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  if (height > kMaxTreeDepth) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "subtree height must be in [0, 20] (0: automatic)");
  ctx->demux_height = height;
  return TFHE_OK;
}

int tfhe_debug_demux_plan(tfhe_context* ctx, size_t trees, size_t depth, unsigned* subtree_height, unsigned* launches) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {subtree_height, launches}, 1, "null pointer"));
  if (trees == 0 || trees > kMaxBatch || depth > kMaxTreeDepth)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "trees must be in [1, 2^31), depth in [0, 20]");
  passes::TreePlan plan{};
  TFHE_TRY(tree_plan_of(ctx, true, trees, depth, &plan));
  *subtree_height = plan.height;
  *launches = plan.launches;
  return TFHE_OK;
}

int tfhe_demux_tree_device(tfhe_context* ctx, const void* selectors_prepared, size_t queries, size_t depth,
                           const uint32_t* glwe_in, size_t values, uint32_t* leaves_out, size_t leaf_sets, int accumulate) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_demux_args(ctx, selectors_prepared, glwe_in, leaves_out, queries, depth, kMaxTreeDepth, leaf_sets, values,
                            accumulate != 0));
  return run_demux(ctx, selectors_prepared, queries, depth, 0, depth, glwe_in, values, leaves_out, leaf_sets == 1 && queries > 1,
                   accumulate != 0);
}

int tfhe_table_write_device(tfhe_context* ctx, const void* selectors_prepared, size_t queries, size_t depth,
                            const uint32_t* values, uint32_t* table_inout, size_t table_sets, size_t tables) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_demux_args(ctx, selectors_prepared, values, table_inout, queries, depth, ctx->pbs.log_n + kMaxTreeDepth,
                            table_sets, tables, true));
  const size_t d_lo = std::min(depth, (size_t)ctx->pbs.log_n);
  return run_demux(ctx, selectors_prepared, queries, depth, d_lo, depth - d_lo, values, tables, table_inout,
                   table_sets == 1 && queries > 1, true);
}

int tfhe_table_lookup_glwe_device(tfhe_context* ctx, const void* selectors_prepared, size_t queries, size_t depth,
                                  const uint32_t* leaves, size_t leaf_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lookup_args(ctx, selectors_prepared, leaves, lwe_out, queries, depth, ctx->pbs.log_n + kMaxTreeDepth, leaf_sets, tables));
  const size_t d_lo = std::min(depth, (size_t)ctx->pbs.log_n);
  return run_lookup(ctx, selectors_prepared, queries, depth, d_lo, depth - d_lo, LookupLeaves{leaves, nullptr, leaf_sets == 1 && queries > 1},
                    tables, nullptr, lwe_out);
}

// host forms: selectors [queries][depth][R][k+1][N] raw; everything uploaded, the selectors prepared once
static int demux_host(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t depth, const uint32_t* in, size_t values,
                      uint32_t* out, size_t sets, bool is_write, bool accumulate) {
  const size_t d_lo = is_write ? std::min(depth, (size_t)ctx->pbs.log_n) : 0;
  const size_t trees = queries * values, glwe = glwe_words(ctx);
  const size_t out_words = ((sets * values) << (depth - d_lo)) * glwe;
  if (overlap(in, trees * glwe, out, out_words)) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the output overlaps the input");
  passes::TreePlan plan{};
  TFHE_TRY(tree_plan_of(ctx, true, trees, depth - d_lo, &plan));
  TFHE_TRY(grow_demux_workspace(ctx, std::max<size_t>(plan.workspace_words, 1)));
  enum { kIn, kOut };
  Staging s(ctx, {trees * glwe, out_words});
  TFHE_TRY(s.reserve());
  TFHE_TRY(upload_and_prepare_ggsw(ctx, selectors, queries * depth));
  TFHE_TRY(s.upload(kIn, in));
  if (accumulate) TFHE_TRY(s.upload(kOut, out));
  TFHE_TRY(is_write ? tfhe_table_write_device(ctx, ctx->d_ggsw_tmp.as(), queries, depth, s[kIn], s[kOut], sets, values)
                    : tfhe_demux_tree_device(ctx, ctx->d_ggsw_tmp.as(), queries, depth, s[kIn], values, s[kOut], sets, accumulate));
  return s.download_and_wait(kOut, out);
}

int tfhe_demux_tree(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t depth, const uint32_t* glwe_in,
                    size_t values, uint32_t* leaves_out, size_t leaf_sets, int accumulate) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_demux_args(ctx, selectors, glwe_in, leaves_out, queries, depth, kMaxTreeDepth, leaf_sets, values, accumulate != 0));
  return demux_host(ctx, selectors, queries, depth, glwe_in, values, leaves_out, leaf_sets, false, accumulate != 0);
}

int tfhe_table_write(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t depth, const uint32_t* values,
                     uint32_t* table_inout, size_t table_sets, size_t tables) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_demux_args(ctx, selectors, values, table_inout, queries, depth, ctx->pbs.log_n + kMaxTreeDepth, table_sets,
                            tables, true));
  return demux_host(ctx, selectors, queries, depth, values, tables, table_inout, table_sets, true, true);
}

int tfhe_table_lookup_glwe(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t depth, const uint32_t* leaves,
                           size_t leaf_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lookup_args(ctx, selectors, leaves, lwe_out, queries, depth, ctx->pbs.log_n + kMaxTreeDepth, leaf_sets, tables));
  const size_t d_hi = depth - std::min(depth, (size_t)ctx->pbs.log_n);
  const size_t trees = queries * tables;
  passes::TreePlan plan{};
  TFHE_TRY(tree_plan_of(ctx, false, trees, d_hi, &plan));
  TFHE_TRY(grow_lookup_workspace(ctx, std::max<size_t>(plan.workspace_words, 1)));
  enum { kIn, kOut };
  Staging s(ctx, {((leaf_sets * tables) << d_hi) * glwe_words(ctx), trees * big_lwe_words(ctx)});
  TFHE_TRY(s.reserve());
  TFHE_TRY(upload_and_prepare_ggsw(ctx, selectors, queries * depth));
  TFHE_TRY(s.upload(kIn, leaves));
  TFHE_TRY(tfhe_table_lookup_glwe_device(ctx, ctx->d_ggsw_tmp.as(), queries, depth, s[kIn], leaf_sets, tables, s[kOut]));
  return s.download_and_wait(kOut, lwe_out);
}

// ---------------------------------------------------------------------------------- encrypted branching program
// include/tfhe_hip.h states the operations, pbs_wave.h::cmux_program_team the run of one team, passes.h the level
// sort, the image, the plan and the passes.
namespace {

using passes::program_image_need;
static_assert(sizeof(tfhe_program_node) == 4 * sizeof(u32), "passes.h reads the nodes as [n_nodes][4] words");

struct ProgramArgs {
  size_t queries, n_inputs, selector_sets;
  const tfhe_program_node* nodes;
  size_t n_nodes, n_terminals;
  const uint32_t* outputs;
  size_t n_outputs;
};

// everything about a program that can be refused without looking at the device
int check_program(tfhe_context* ctx, const ProgramArgs& a) {
  if (a.queries == 0 || a.queries > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries must be in [1, 2^31)");
  if (a.selector_sets != 1 && a.selector_sets != a.queries)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "selector_sets must be 1 or queries");
  if (a.n_outputs == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "n_outputs must be at least 1");
  if (a.n_terminals == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "n_terminals must be at least 1");
  if (a.n_nodes > 0 && (!a.nodes || a.n_inputs == 0)) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "nodes without a node array or without inputs");
  if (a.n_inputs > kMaxBatch || a.n_terminals > kMaxBatch || a.n_nodes > kMaxBatch || a.n_outputs > kMaxBatch ||
      a.n_terminals + a.n_nodes > kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "n_inputs, n_terminals + n_nodes and n_outputs must be below 2^31");
  for (size_t i = 0; i < a.n_nodes; ++i) {
    const tfhe_program_node& n = a.nodes[i];
    const std::string at = "node " + std::to_string(i) + ": ";
    if (n.sel >= a.n_inputs) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, at + "sel " + std::to_string(n.sel) + " is not below n_inputs");
    if (n.rot >= 2 * ctx->N) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, at + "rot " + std::to_string(n.rot) + " is not below 2N");
    if (n.lo >= a.n_terminals + i || n.hi >= a.n_terminals + i)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, at + "a node may only reference terminals and earlier nodes (forward or self reference)");
  }
  for (size_t o = 0; o < a.n_outputs; ++o)
    if (a.outputs[o] >= a.n_terminals + a.n_nodes)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "output " + std::to_string(o) + " references neither a terminal nor a node");
  return TFHE_OK;
}

// passes.h::program_levels of the call's nodes
void program_levels(const ProgramArgs& a, std::vector<u32>* level_counts, std::vector<u32>* order) {
  passes::program_levels(reinterpret_cast<const u32*>(a.nodes), a.n_nodes, a.n_terminals, level_counts, order);
}

size_t program_bytes(const tfhe_context* ctx, size_t queries, size_t nodes, size_t outputs) {
  return (queries * nodes * glwe_words(ctx) + tfhe_context::kProgramImages * program_image_need(nodes, outputs)) * sizeof(u32);
}

int plan_program_of(tfhe_context* ctx, size_t queries, const std::vector<u32>& counts, size_t n_outputs,
                    std::vector<passes::ProgramLaunch>* launches, passes::ProgramPlan* info) {
  launches->resize(counts.size() + 1);
  unsigned resident = 0;
  hipError_t e = launch::program_resident_teams(ctx->field, ctx->pbs, &resident);
  if (e == hipSuccess && !passes::program_plan_for(queries, counts.data(), (u32)counts.size(), (u32)n_outputs, ctx->program_parts,
                                                   resident, launches->data(), info))
    e = hipErrorInvalidValue;
  if (e == hipErrorInvalidValue)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries * teams per query exceeds the 2^31 - 1 teams of one launch");
  if (e != hipSuccess) return hip_fail(ctx, e, "program plan");
  launches->resize(info->launches);
  return TFHE_OK;
}

int reserve_program(tfhe_context* ctx, size_t queries, size_t nodes, size_t outputs) {
  const size_t values = std::max<size_t>(1, queries * nodes * glwe_words(ctx)), image = program_image_need(nodes, outputs);
  if (values <= ctx->program_value_words && image <= ctx->program_image_words) return TFHE_OK;
  const size_t new_values = std::max(values, ctx->program_value_words), new_image = std::max(image, ctx->program_image_words);
  for (auto& im : ctx->program_images) im = tfhe_context::ProgramImage{};
  ctx->program_value_words = ctx->program_image_words = 0;
  TFHE_TRY(ctx->d_program_ws.grow(ctx, (new_values + tfhe_context::kProgramImages * new_image) * sizeof(u32)));
  ctx->program_value_words = new_values;
  ctx->program_image_words = new_image;
  return TFHE_OK;
}

// the resident image of the program, uploaded if this is its first use
int program_image(tfhe_context* ctx, const ProgramArgs& a, u32** d_image, const std::vector<u32>** counts) {
  std::vector<u32> key;
  key.reserve(4 + a.n_nodes * 4 + a.n_outputs);
  for (size_t v : {a.n_inputs, a.n_terminals, a.n_nodes, a.n_outputs}) key.push_back((u32)v);
  for (size_t i = 0; i < a.n_nodes; ++i)
    for (u32 v : {a.nodes[i].sel, a.nodes[i].lo, a.nodes[i].hi, a.nodes[i].rot}) key.push_back(v);
  key.insert(key.end(), a.outputs, a.outputs + a.n_outputs);
  tfhe_context::ProgramImage* slot = nullptr;
  for (auto& im : ctx->program_images)
    if (im.key == key) slot = &im;
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(ctx->stream, &capture) != hipSuccess || capture != hipStreamCaptureStatusNone;
  if (!slot) {
    if (capturing)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                  "first use of this program during a stream capture: its upload synchronises, run the program once before capturing");
    for (auto& im : ctx->program_images)
      if (!im.pinned && (!slot || im.last_use < slot->last_use)) slot = &im;
    if (!slot)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                  "every program image of the context is held by a captured graph; tfhe_context_reserve_program with a larger "
                  "need releases them (and voids those graphs)");
    std::vector<u32> order, level_counts;
    program_levels(a, &level_counts, &order);
    std::vector<u32> image(program_image_need(a.n_nodes, a.n_outputs));
    passes::program_image(reinterpret_cast<const u32*>(a.nodes), order, a.outputs, a.n_outputs, image.data());
    slot->key.clear();  // not a valid entry until the upload has succeeded
    u32* dst = ctx->d_program_ws.as<u32>() + ctx->program_value_words + (size_t)(slot - ctx->program_images) * ctx->program_image_words;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches of the image this one replaces may be in flight
    HIP_TRY(ctx, hipMemcpy(dst, image.data(), image.size() * sizeof(u32), hipMemcpyHostToDevice));
    slot->key = std::move(key);
    slot->level_counts = std::move(level_counts);
  }
  slot->last_use = ++ctx->program_clock;
  if (capturing) slot->pinned = true;
  *d_image = ctx->d_program_ws.as<u32>() + ctx->program_value_words + (size_t)(slot - ctx->program_images) * ctx->program_image_words;
  *counts = &slot->level_counts;
  return TFHE_OK;
}

}  // namespace

int tfhe_context_reserve_program(tfhe_context* ctx, size_t max_queries, size_t max_nodes, size_t max_outputs) {
  TFHE_TRY(check_ctx(ctx));
  if (max_queries == 0 || max_queries > kMaxBatch || max_nodes > kMaxBatch || max_outputs == 0 || max_outputs > kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_queries and max_outputs must be in [1, 2^31), max_nodes below 2^31");
  return reserve_program(ctx, max_queries, max_nodes, max_outputs);
}

int tfhe_context_set_program_split(tfhe_context* ctx, unsigned parts) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  if (parts > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "parts must be below 2^31 (0: automatic)");
  ctx->program_parts = parts;
  return TFHE_OK;
}

int tfhe_debug_program_plan(tfhe_context* ctx, size_t queries, const tfhe_program_node* nodes, size_t n_nodes, size_t n_terminals,
                            unsigned* launches, unsigned* teams_per_query) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {launches, teams_per_query}, 1, "null pointer"));
  const uint32_t out0 = 0;
  ProgramArgs a{queries, kMaxBatch, 1, nodes, n_nodes, n_terminals, &out0, 1};
  TFHE_TRY(check_program(ctx, a));
  std::vector<passes::ProgramLaunch> plan;
  passes::ProgramPlan info{};
  std::vector<u32> counts;
  program_levels(a, &counts, nullptr);
  TFHE_TRY(plan_program_of(ctx, queries, counts, 1, &plan, &info));
  *launches = info.launches;
  *teams_per_query = info.teams_per_query;
  return TFHE_OK;
}

int tfhe_cmux_program_device(tfhe_context* ctx, const void* selectors_prepared, size_t queries, size_t n_inputs, size_t selector_sets,
                             const tfhe_program_node* nodes, size_t n_nodes, const uint32_t* terminals, size_t n_terminals,
                             const uint32_t* outputs, size_t n_outputs, uint32_t* glwe_out, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {terminals, outputs}, 1, "null pointer"));
  if (!glwe_out && !lwe_out) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "glwe_out and lwe_out are both null");
  if (n_nodes > 0 && !selectors_prepared) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer");
  const ProgramArgs a{queries, n_inputs, selector_sets, nodes, n_nodes, n_terminals, outputs, n_outputs};
  TFHE_TRY(check_program(ctx, a));
  if (std::max<size_t>(1, queries * n_nodes * glwe_words(ctx)) > ctx->program_value_words ||
      program_image_need(n_nodes, n_outputs) > ctx->program_image_words)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(program_bytes(ctx, queries, n_nodes, n_outputs)) + " bytes of program workspace (" +
                    std::to_string(queries) + " queries, " + std::to_string(n_nodes) + " nodes, " + std::to_string(n_outputs) +
                    " outputs), " + std::to_string(ctx->d_program_ws.bytes()) + " are reserved (tfhe_context_reserve_program)");
  u32* d_image = nullptr;
  const std::vector<u32>* counts = nullptr;
  TFHE_TRY(program_image(ctx, a, &d_image, &counts));
  std::vector<passes::ProgramLaunch> plan;
  passes::ProgramPlan info{};
  TFHE_TRY(plan_program_of(ctx, queries, *counts, n_outputs, &plan, &info));
  const passes::ProgramCall call{selectors_prepared, selector_sets == 1 ? 0 : n_inputs * prepared_ggsw_words(ctx), d_image, terminals,
                                 (u32)n_terminals, (u32)n_nodes, (u32)n_outputs, ctx->d_program_ws.as<u32>(), glwe_out, lwe_out};
  return passes::program_passes(plan.data(), plan.size(), call, [&](const CmuxProgramPass& pass) {
    HIP_TRY(ctx, launch::cmux_program_pass(ctx->stream, ctx->field, ctx->pbs, ctx->d_tw.as(), pass, queries));
    return (int)TFHE_OK;
  });
}

// host form: selectors [selector_sets][n_inputs][R][k+1][N] raw; everything uploaded, the selectors prepared once
int tfhe_cmux_program(tfhe_context* ctx, const uint32_t* selectors, size_t queries, size_t n_inputs, size_t selector_sets,
                      const tfhe_program_node* nodes, size_t n_nodes, const uint32_t* terminals, size_t n_terminals,
                      const uint32_t* outputs, size_t n_outputs, uint32_t* glwe_out, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {terminals, outputs}, 1, "null pointer"));
  if (!glwe_out && !lwe_out) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "glwe_out and lwe_out are both null");
  if (n_nodes > 0 && !selectors) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer");
  TFHE_TRY(check_program(ctx, ProgramArgs{queries, n_inputs, selector_sets, nodes, n_nodes, n_terminals, outputs, n_outputs}));
  TFHE_TRY(reserve_program(ctx, queries, n_nodes, n_outputs));
  enum { kTerminals, kGlwe, kLwe };
  Staging s(ctx, {n_terminals * ctx->N, glwe_out ? queries * n_outputs * glwe_words(ctx) : 0, lwe_out ? queries * n_outputs * big_lwe_words(ctx) : 0});
  TFHE_TRY(s.reserve());
  if (n_nodes > 0) TFHE_TRY(upload_and_prepare_ggsw(ctx, selectors, selector_sets * n_inputs));
  TFHE_TRY(s.upload(kTerminals, terminals));
  TFHE_TRY(tfhe_cmux_program_device(ctx, n_nodes > 0 ? ctx->d_ggsw_tmp.as() : nullptr, queries, n_inputs, selector_sets, nodes, n_nodes,
                                    s[kTerminals], n_terminals, outputs, n_outputs, glwe_out ? s[kGlwe] : nullptr,
                                    lwe_out ? s[kLwe] : nullptr));
  if (glwe_out && lwe_out) TFHE_TRY(download(ctx, glwe_out, s[kGlwe], queries * n_outputs * glwe_words(ctx)));
  return lwe_out ? s.download_and_wait(kLwe, lwe_out) : s.download_and_wait(kGlwe, glwe_out);
}

// ---------------------------------------------------------------------------------- small ops
int tfhe_decompose(tfhe_context* ctx, int which, const uint32_t* values, size_t count, uint32_t* digits_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {values, digits_out}, count, "null pointer / zero count"));
  if (which != TFHE_DECOMPOSER_PBS && which != TFHE_DECOMPOSER_KS) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "bad decomposer selector");
  const tfhe_decomposer_params& d = which == TFHE_DECOMPOSER_PBS ? ctx->params.pbs_decomposer : ctx->params.ks_decomposer;
  enum { kIn, kOut };
  Staging s(ctx, {count, count * d.levels});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, values));
  HIP_TRY(ctx, launch::decompose_words(ctx->stream, d.log_base, d.levels,
                                       gadget_top(ctx, d.log_base) - d.log_base * d.levels, s[kIn], count, s[kOut]));
  return s.download_and_wait(kOut, digits_out);
}

int tfhe_decompose_glwe_batch(tfhe_context* ctx, const uint32_t* glwe, size_t batch, uint32_t* digits_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe, digits_out}, batch));
  const u32 polys = ctx->params.glwe_dimension + 1;
  enum { kIn, kOut };
  Staging s(ctx, {batch * glwe_words(ctx), batch * glwe_words(ctx) * ctx->pbs.levels});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, glwe));
  HIP_TRY(ctx, launch::decompose_glwe(ctx->stream, ctx->pbs.log_base, ctx->pbs.levels, ctx->pbs.first_shift, polys, ctx->N, s[kIn], batch, s[kOut]));
  return s.download_and_wait(kOut, digits_out);
}

int tfhe_switch_modulus(tfhe_context* ctx, const uint32_t* values, size_t count, uint32_t log_from,
                        uint32_t log_to, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {values, out}, count, "null pointer / zero count"));
  // `1 << (log_from - log_to)` and `1 << log_to` on u32 (utils.rs:27-28)
  if (log_from > 32 || log_to > log_from || log_from - log_to >= 32 || log_to >= 32)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "switch_modulus shift out of range");
  enum { kIn, kOut };
  Staging s(ctx, {count, count});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, values));
  HIP_TRY(ctx, launch::switch_modulus(ctx->stream, s[kIn], count, log_from, log_to, s[kOut]));
  return s.download_and_wait(kOut, out);
}

int tfhe_glwe_mul_monomial_batch(tfhe_context* ctx, const uint32_t* glwe_in, size_t batch,
                                 const int64_t* monomial_index, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe_in, monomial_index, glwe_out}, batch));
  const size_t w = batch * glwe_words(ctx);
  enum { kIndex, kIn, kOut };  // the 8-byte indices first, in a segment of whole 16-byte units
  Staging s(ctx, {(batch * sizeof(i64) + 15) / 16 * 4, w, w});
  TFHE_TRY(s.reserve());
  HIP_TRY(ctx, hipMemcpyAsync(s[kIndex], monomial_index, batch * sizeof(i64), hipMemcpyHostToDevice, ctx->stream));
  TFHE_TRY(s.upload(kIn, glwe_in));
  HIP_TRY(ctx, launch::glwe_mul_monomial(ctx->stream, ctx->pbs.log_n, ctx->params.glwe_dimension + 1, s[kIn], batch,
                                         reinterpret_cast<const i64*>(s[kIndex]), s[kOut]));
  return s.download_and_wait(kOut, glwe_out);
}

// ---------------------------------------------------------------------------------- lwe.rs
namespace {
int check_lwe_linear_args(tfhe_context* ctx, const void* ct0, uint32_t c1, const void* ct1, size_t batch, size_t words_per_ct,
                          const void* out) {
  if (!ct0 || !out || batch == 0 || words_per_ct == 0 || (c1 != 0 && !ct1))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer / empty batch");
  return TFHE_OK;
}
}  // namespace

int tfhe_lwe_linear_batch_device(tfhe_context* ctx, uint32_t c0, const uint32_t* ct0, uint32_t c1,
                                 const uint32_t* ct1, size_t batch, size_t words_per_ct, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lwe_linear_args(ctx, ct0, c1, ct1, batch, words_per_ct, out));
  HIP_TRY(ctx, launch::lwe_linear(ctx->stream, c0, ct0, c1, c1 ? ct1 : nullptr, batch * words_per_ct, out));
  return TFHE_OK;
}

int tfhe_lwe_linear_batch(tfhe_context* ctx, uint32_t c0, const uint32_t* ct0, uint32_t c1,
                          const uint32_t* ct1, size_t batch, size_t words_per_ct, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_lwe_linear_args(ctx, ct0, c1, ct1, batch, words_per_ct, out));
  const size_t words = batch * words_per_ct;
  enum { kCt0, kCt1, kOut };
  Staging s(ctx, {words, words, words});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kCt0, ct0));
  if (c1) TFHE_TRY(s.upload(kCt1, ct1));
  TFHE_TRY(tfhe_lwe_linear_batch_device(ctx, c0, s[kCt0], c1, c1 ? s[kCt1] : nullptr, batch, words_per_ct, s[kOut]));
  return s.download_and_wait(kOut, out);
}

// ---------------------------------------------------------------------------------- encrypted dense layers
// include/tfhe_hip.h states the operations, lwe_dense.h::dense_tile the tiling, kernels.hip::dense_plan_for the plan.
namespace {

struct DenseShape {
  size_t queries, inputs, outputs, words;
};

// everything about a dense call that can be refused without looking at the device; -> the plan
int check_dense(tfhe_context* ctx, const DenseShape& d, launch::DensePlanInfo* plan) {
  if (d.queries == 0 || d.inputs == 0 || d.outputs == 0 || d.words == 0)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries, inputs, outputs and words_per_ct must be at least 1");
  if (d.queries > kMaxBatch || d.inputs > kMaxBatch || d.outputs > kMaxBatch || d.words > kMaxBatch ||
      !launch::dense_plan(d.queries, (u32)d.inputs, (u32)d.outputs, (u32)d.words, ctx->dense_parts, plan))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the tiles of the call exceed one grid: queries * ceil(words_per_ct / 128) and inputs must be below 2^31, outputs at "
                "most 32 * 65535");
  return TFHE_OK;
}

int check_dense_args(tfhe_context* ctx, const void* x, const void* w, const void* out, const DenseShape& d,
                     launch::DensePlanInfo* plan) {
  TFHE_TRY(check_present(ctx, {x, w, out}, 1, "null pointer"));
  return check_dense(ctx, d, plan);
}

int enqueue_dense(tfhe_context* ctx, const u32* x, const DenseShape& d, const int32_t* w, const u32* bias, u32* out) {
  HIP_TRY(ctx, launch::lwe_dense(ctx->stream, x, d.queries, (u32)d.inputs, w, bias, (u32)d.outputs, (u32)d.words, ctx->dense_parts, out));
  return TFHE_OK;
}

// The fused layer's workspace: [pre-activations: one ciphertext per bootstrap][test vectors: [N] per bootstrap], the
// first at the larger boundary dimension so that switching the bootstrap order keeps a reservation valid
size_t dense_row_words(const tfhe_context* ctx) { return std::max(lwe_words(ctx), big_lwe_words(ctx)) + ctx->N; }

int reserve_dense(tfhe_context* ctx, size_t rows) {
  TFHE_TRY(reserve(ctx, rows));
  if (rows <= ctx->dense_rows) return TFHE_OK;
  ctx->dense_rows = 0;
  TFHE_TRY(ctx->d_dense_ws.grow(ctx, rows * dense_row_words(ctx) * sizeof(u32)));
  ctx->dense_rows = rows;
  return TFHE_OK;
}

int check_dense_bootstrap_args(tfhe_context* ctx, const void* x, const void* w, const void* tv, const void* out, const DenseShape& d,
                               size_t tv_count, launch::DensePlanInfo* plan) {
  TFHE_TRY(check_present(ctx, {x, w, tv, out}, 1, "null pointer"));
  TFHE_TRY(check_dense(ctx, d, plan));
  if (tv_count != 1 && tv_count != d.outputs) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "tv_count must be 1 or outputs");
  if ((double)d.queries * (double)d.outputs > (double)kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries * outputs exceeds 2^31 - 1 (one workgroup per bootstrap)");
  // the bootstraps' own refusals (a key, what the loaded key supports), as tfhe_bootstrap_batch states them
  return check_rotate_args(ctx, x, tv, out, d.queries * d.outputs, 1);
}

}  // namespace

int tfhe_context_reserve_dense(tfhe_context* ctx, size_t max_queries, size_t max_outputs) {
  TFHE_TRY(check_ctx(ctx));
  if (max_queries == 0 || max_outputs == 0 || (double)max_queries * (double)max_outputs > (double)kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_queries and max_outputs must be at least 1, their product below 2^31");
  return reserve_dense(ctx, max_queries * max_outputs);
}

int tfhe_context_set_dense_split(tfhe_context* ctx, unsigned parts) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  if (parts > 65535u) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "parts must be at most 65535 (0: automatic)");
  ctx->dense_parts = parts;
  return TFHE_OK;
}

int tfhe_debug_dense_plan(tfhe_context* ctx, size_t queries, size_t inputs, size_t outputs, size_t words_per_ct, unsigned* splits,
                          unsigned* workgroups) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {splits, workgroups}, 1, "null pointer"));
  launch::DensePlanInfo plan{};
  TFHE_TRY(check_dense(ctx, DenseShape{queries, inputs, outputs, words_per_ct}, &plan));
  *splits = plan.splits;
  *workgroups = (unsigned)std::min<size_t>(plan.workgroups, 0xFFFFFFFFu);
  return TFHE_OK;
}

int tfhe_lwe_dense_batch_device(tfhe_context* ctx, const uint32_t* x, size_t queries, size_t inputs, const int32_t* weights,
                                const uint32_t* bias, size_t outputs, size_t words_per_ct, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  const DenseShape d{queries, inputs, outputs, words_per_ct};
  launch::DensePlanInfo plan{};
  TFHE_TRY(check_dense_args(ctx, x, weights, out, d, &plan));
  if (overlap(out, queries * outputs * words_per_ct, x, queries * inputs * words_per_ct))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "out overlaps x: every output reads every input of its query");
  return enqueue_dense(ctx, x, d, weights, bias, out);
}

int tfhe_lwe_dense_batch(tfhe_context* ctx, const uint32_t* x, size_t queries, size_t inputs, const int32_t* weights,
                         const uint32_t* bias, size_t outputs, size_t words_per_ct, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  const DenseShape d{queries, inputs, outputs, words_per_ct};
  launch::DensePlanInfo plan{};
  TFHE_TRY(check_dense_args(ctx, x, weights, out, d, &plan));
  if (overlap(out, queries * outputs * words_per_ct, x, queries * inputs * words_per_ct))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "out overlaps x: every output reads every input of its query");
  enum { kX, kW, kBias, kOut };
  Staging s(ctx, {queries * inputs * words_per_ct, outputs * inputs, bias ? outputs : 0, queries * outputs * words_per_ct});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kX, x));
  TFHE_TRY(s.upload(kW, weights));
  if (bias) TFHE_TRY(s.upload(kBias, bias));
  TFHE_TRY(enqueue_dense(ctx, s[kX], d, reinterpret_cast<const int32_t*>(s[kW]), bias ? s[kBias] : nullptr, s[kOut]));
  return s.download_and_wait(kOut, out);
}

int tfhe_dense_bootstrap_batch_device(tfhe_context* ctx, const uint32_t* x, size_t queries, size_t inputs, const int32_t* weights,
                                      const uint32_t* bias, size_t outputs, const uint32_t* test_vector_poly, size_t tv_count,
                                      uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  const DenseShape d{queries, inputs, outputs, io_words(ctx)};
  launch::DensePlanInfo plan{};
  TFHE_TRY(check_dense_bootstrap_args(ctx, x, weights, test_vector_poly, lwe_out, d, tv_count, &plan));
  const size_t rows = queries * outputs;
  if (rows > ctx->dense_rows || rows > ctx->ws_batch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(rows * dense_row_words(ctx) * sizeof(u32)) + " bytes of dense workspace (" +
                    std::to_string(queries) + " queries, " + std::to_string(outputs) + " outputs), " +
                    std::to_string(ctx->dense_rows * dense_row_words(ctx) * sizeof(u32)) +
                    " are reserved (tfhe_context_reserve_dense)");
  u32* pre = ctx->d_dense_ws.as<u32>();
  u32* tvs = ctx->d_dense_ws.as<u32>() + ctx->dense_rows * (dense_row_words(ctx) - ctx->N);
  TFHE_TRY(enqueue_dense(ctx, x, d, weights, bias, pre));
  const u32* tv = test_vector_poly;
  if (tv_count != 1) {  // the rotation reads bootstrap r's test vector at r * N: neuron r % O's
    HIP_TRY(ctx, launch::dense_tile_rows(ctx->stream, test_vector_poly, outputs, rows, ctx->N, tvs));
    tv = tvs;
  }
  return enqueue_bootstrap(ctx, pre, rows, tv, tv_count == 1 ? 1 : rows, ctx->d_lwe_big.as<u32>(), lwe_out);
}

int tfhe_dense_bootstrap_batch(tfhe_context* ctx, const uint32_t* x, size_t queries, size_t inputs, const int32_t* weights,
                               const uint32_t* bias, size_t outputs, const uint32_t* test_vector_poly, size_t tv_count,
                               uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  const size_t io = io_words(ctx);
  launch::DensePlanInfo plan{};
  TFHE_TRY(check_dense_bootstrap_args(ctx, x, weights, test_vector_poly, lwe_out, DenseShape{queries, inputs, outputs, io}, tv_count, &plan));
  TFHE_TRY(check_tv_host(ctx, test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(reserve_dense(ctx, queries * outputs));
  enum { kX, kW, kBias, kTv, kOut };
  Staging s(ctx, {queries * inputs * io, outputs * inputs, bias ? outputs : 0, tv_count * ctx->N, queries * outputs * io});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kX, x));
  TFHE_TRY(s.upload(kW, weights));
  if (bias) TFHE_TRY(s.upload(kBias, bias));
  TFHE_TRY(s.upload(kTv, test_vector_poly));
  TFHE_TRY(tfhe_dense_bootstrap_batch_device(ctx, s[kX], queries, inputs, reinterpret_cast<const int32_t*>(s[kW]),
                                             bias ? s[kBias] : nullptr, outputs, s[kTv], tv_count, s[kOut]));
  return s.download_and_wait(kOut, lwe_out);
}

// ---------------------------------------------------------------------------------- encrypted convolutions
// include/tfhe_hip.h states the operation, glwe_conv.h::glwe_conv_team the team and its exactness bound.
namespace {

constexpr ExactnessNouns kConvNouns = {"weight_bits", "rows_per_pass", "pass"};

// The most channels this backend sums exactly in one pass at weights of magnitude 2^bits, or 0 with the reason in *why.
// exactness_refusal is monotone in the rows, so the largest admitted count is found by bisection.
unsigned conv_rows_admitted(const tfhe_context* ctx, int bits, std::string* why) {
  *why = exactness_refusal(ctx, 1, bits, kConvNouns);
  if (!why->empty()) return 0;
  unsigned lo = 1, hi = (1u << 20) + 1;  // admitted, not admitted (beyond every field's kMaxRows)
  while (hi - lo > 1) {
    const unsigned mid = lo + (hi - lo) / 2;
    (exactness_refusal(ctx, (int)mid, bits, kConvNouns).empty() ? lo : hi) = mid;
  }
  return lo;
}

size_t conv_poly_bytes(const tfhe_context* ctx) { return (size_t)ctx->parts * ctx->N * sizeof(u64); }  // one prepared polynomial

int reserve_conv(tfhe_context* ctx, size_t polys) {
  if (polys <= ctx->conv_ws_polys) return TFHE_OK;
  ctx->conv_ws_polys = 0;
  TFHE_TRY(ctx->d_conv_ws.grow(ctx, polys * conv_poly_bytes(ctx)));
  ctx->conv_ws_polys = polys;
  return TFHE_OK;
}

// everything about a convolution that can be refused on the host; -> the plan
int check_conv(tfhe_context* ctx, const tfhe_poly_weights* w, size_t queries, launch::GlweConvPlanInfo* plan) {
  if (!w) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null weights");
  if (w->device != ctx->device || w->field != ctx->field || w->log_n != ctx->pbs.log_n)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the weights were prepared by a context of another device, backend or ring degree");
  if (queries == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries must be at least 1");
  if (ctx->conv_rows > w->rows_per_pass)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "tfhe_context_set_glwe_conv_rows(" + std::to_string(ctx->conv_rows) + ") exceeds the " + std::to_string(w->rows_per_pass) +
                    " rows per pass the backend admits at weight_bits = " + std::to_string(w->weight_bits));
  if (queries > kMaxBatch ||
      !launch::glwe_conv_plan(queries, (u32)w->channels, (u32)w->outputs, w->rows_per_pass, ctx->conv_rows, plan))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries * outputs exceeds 2^31 - 1 (one workgroup per output ciphertext)");
  if ((double)queries * (double)w->channels * (double)(ctx->params.glwe_dimension + 1) > (double)kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "queries * channels * (k+1) exceeds 2^31 - 1");
  return TFHE_OK;
}

int check_conv_args(tfhe_context* ctx, const u32* x, const tfhe_poly_weights* w, const u32* out, size_t queries,
                    launch::GlweConvPlanInfo* plan) {
  TFHE_TRY(check_present(ctx, {x, out}, 1, "null pointer"));
  TFHE_TRY(check_conv(ctx, w, queries, plan));
  if (overlap(out, queries * w->outputs * glwe_words(ctx), x, queries * w->channels * glwe_words(ctx)))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "out overlaps x: every output reads every channel of its query");
  return TFHE_OK;
}

}  // namespace

int tfhe_prepare_poly_weights(tfhe_context* ctx, const int32_t* weights, size_t outputs, size_t channels, tfhe_poly_weights** out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {weights, out}, 1, "null pointer"));
  *out = nullptr;
  if (outputs == 0 || channels == 0 || outputs > kMaxBatch || channels > kMaxBatch ||
      (double)outputs * (double)channels > (double)kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "outputs and channels must be at least 1, their product below 2^31");
  const size_t polys = outputs * channels, words = polys * ctx->N;
  int64_t largest = 0;
  for (size_t i = 0; i < words; ++i) largest = std::max<int64_t>(largest, std::llabs((long long)weights[i]));
  int bits = 0;
  while (((int64_t)1 << bits) < largest) ++bits;
  std::string why;
  const unsigned rows = conv_rows_admitted(ctx, bits, &why);
  if (rows == 0) return fail(ctx, TFHE_ERR_EXACTNESS, "polynomial weights refused: " + why);
  tfhe_poly_weights* w = new (std::nothrow) tfhe_poly_weights();
  if (!w) return fail(ctx, TFHE_ERR_HIP, "out of host memory");
  w->device = ctx->device;
  w->field = ctx->field;
  w->log_n = ctx->pbs.log_n;
  w->outputs = outputs;
  w->channels = channels;
  w->weight_bits = (unsigned)bits;
  w->rows_per_pass = rows;
  DeviceBuffer raw;
  int st = raw.grow(ctx, words * sizeof(u32));
  if (st == TFHE_OK) st = w->d_spec.grow(ctx, polys * (size_t)ctx->N * sizeof(u64));
  if (st == TFHE_OK) {
    hipError_t e = hipMemcpyAsync(raw.as(), weights, words * sizeof(u32), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
      e = launch::conv_weights(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->d_tw.as(), raw.as<const i32>(), polys, w->d_spec.as());
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the staging buffer goes away with this call
    if (e != hipSuccess) st = hip_fail(ctx, e, "tfhe_prepare_poly_weights");
  }
  if (st != TFHE_OK) {
    tfhe_poly_weights_destroy(w);
    return st;
  }
  *out = w;
  return TFHE_OK;
}

void tfhe_poly_weights_destroy(tfhe_poly_weights* weights) {
  if (!weights) return;
  (void)hipSetDevice(weights->device);  // before `delete` releases the spectra
  delete weights;
}

int tfhe_poly_weights_info(const tfhe_poly_weights* weights, size_t* outputs, size_t* channels, unsigned* weight_bits,
                           unsigned* rows_per_pass) {
  if (!weights) return TFHE_ERR_INVALID_ARGUMENT;
  if (outputs) *outputs = weights->outputs;
  if (channels) *channels = weights->channels;
  if (weight_bits) *weight_bits = weights->weight_bits;
  if (rows_per_pass) *rows_per_pass = weights->rows_per_pass;
  return TFHE_OK;
}

int tfhe_context_reserve_glwe_conv(tfhe_context* ctx, size_t max_queries, size_t max_channels) {
  TFHE_TRY(check_ctx(ctx));
  if (max_queries == 0 || max_channels == 0 ||
      (double)max_queries * (double)max_channels * (double)(ctx->params.glwe_dimension + 1) > (double)kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "max_queries and max_channels must be at least 1, their product times k+1 below 2^31");
  return reserve_conv(ctx, max_queries * max_channels * (ctx->params.glwe_dimension + 1));
}

int tfhe_context_set_glwe_conv_rows(tfhe_context* ctx, unsigned rows) {
  if (!ctx) return TFHE_ERR_INVALID_ARGUMENT;
  std::string why;
  const unsigned most = conv_rows_admitted(ctx, 0, &why);  // what the backend admits for the smallest weights there are
  if (rows > most)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "rows exceeds the " + std::to_string(most) + " rows per pass this backend admits at all (0: automatic)" +
                    (why.empty() ? "" : ": " + why));
  ctx->conv_rows = rows;
  return TFHE_OK;
}

int tfhe_debug_glwe_conv_plan(tfhe_context* ctx, const tfhe_poly_weights* weights, size_t queries, unsigned* rows_per_pass,
                              unsigned* passes, unsigned* teams) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {rows_per_pass, passes, teams}, 1, "null pointer"));
  launch::GlweConvPlanInfo plan{};
  TFHE_TRY(check_conv(ctx, weights, queries, &plan));
  *rows_per_pass = plan.rows_per_pass;
  *passes = plan.passes;
  *teams = (unsigned)plan.teams;
  return TFHE_OK;
}

int tfhe_glwe_conv_batch_device(tfhe_context* ctx, const uint32_t* x, size_t queries, const tfhe_poly_weights* weights,
                                const uint32_t* bias, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  launch::GlweConvPlanInfo plan{};
  TFHE_TRY(check_conv_args(ctx, x, weights, out, queries, &plan));
  const size_t polys = queries * weights->channels * (ctx->params.glwe_dimension + 1);
  if (polys > ctx->conv_ws_polys)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(polys * conv_poly_bytes(ctx)) + " bytes of convolution workspace (" +
                    std::to_string(queries) + " queries, " + std::to_string(weights->channels) + " channels), " +
                    std::to_string(ctx->conv_ws_polys * conv_poly_bytes(ctx)) + " are reserved (tfhe_context_reserve_glwe_conv)");
  HIP_TRY(ctx, launch::bsk_prepare(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->pbs.k, ctx->d_tw.as(), x, polys, ctx->d_conv_ws.as()));
  const GlweConvArgs args{ctx->d_conv_ws.as(), weights->d_spec.as(), bias, out, (u32)weights->channels, (u32)weights->outputs, plan.rows_per_pass};
  HIP_TRY(ctx, launch::glwe_conv(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->pbs.k, ctx->d_tw.as(), args, queries));
  return TFHE_OK;
}

int tfhe_glwe_conv_batch(tfhe_context* ctx, const uint32_t* x, size_t queries, const tfhe_poly_weights* weights,
                         const uint32_t* bias, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  launch::GlweConvPlanInfo plan{};
  TFHE_TRY(check_conv_args(ctx, x, weights, out, queries, &plan));
  TFHE_TRY(reserve_conv(ctx, queries * weights->channels * (ctx->params.glwe_dimension + 1)));
  enum { kX, kBias, kOut };
  Staging s(ctx, {queries * weights->channels * glwe_words(ctx), bias ? weights->outputs * (size_t)ctx->N : 0,
                  queries * weights->outputs * glwe_words(ctx)});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kX, x));
  if (bias) TFHE_TRY(s.upload(kBias, bias));
  TFHE_TRY(tfhe_glwe_conv_batch_device(ctx, s[kX], queries, weights, bias ? s[kBias] : nullptr, s[kOut]));
  return s.download_and_wait(kOut, out);
}

namespace {
int check_extract_indices(tfhe_context* ctx, const void* glwe, const void* indices, const void* lwe_out, size_t batch, size_t count) {
  TFHE_TRY(check_present(ctx, {glwe, indices, lwe_out}, 1, "null pointer"));
  if (batch == 0 || count == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch and count must be at least 1");
  if ((double)batch * (double)count > (double)kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch * count exceeds 2^31 - 1");
  return TFHE_OK;
}
}  // namespace

int tfhe_sample_extract_indices_device(tfhe_context* ctx, const uint32_t* glwe, size_t batch, const uint32_t* indices,
                                       size_t count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_extract_indices(ctx, glwe, indices, lwe_out, batch, count));
  HIP_TRY(ctx, launch::sample_extract_indices(ctx->stream, ctx->pbs.log_n, ctx->pbs.k, glwe, batch, indices, count, lwe_out));
  return TFHE_OK;
}

int tfhe_sample_extract_indices(tfhe_context* ctx, const uint32_t* glwe, size_t batch, const uint32_t* indices, size_t count,
                                uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_extract_indices(ctx, glwe, indices, lwe_out, batch, count));
  for (size_t i = 0; i < count; ++i)
    if (indices[i] >= ctx->N) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "sample index >= N (bootstrapping.rs:127)");
  enum { kIn, kIndex, kOut };
  Staging s(ctx, {batch * glwe_words(ctx), count, batch * count * big_lwe_words(ctx)});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, glwe));
  TFHE_TRY(s.upload(kIndex, indices));
  TFHE_TRY(tfhe_sample_extract_indices_device(ctx, s[kIn], batch, s[kIndex], count, s[kOut]));
  return s.download_and_wait(kOut, lwe_out);
}

// ---------------------------------------------------------------------------------- encryption side
// keygen / encrypt / decrypt with the caller's randomness already in the buffers (tfhe_hip.h)
namespace {

int check_binary(tfhe_context* ctx, const u32* sk, size_t words, const char* what) {
  for (size_t i = 0; i < words; ++i)
    if (sk[i] > 1u)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, std::string(what) + " must be binary (sample_binary)");
  return TFHE_OK;
}

int ensure_key_tmp(tfhe_context* ctx, size_t words) { return ctx->d_key_tmp.grow(ctx, words * sizeof(u32)); }

int to_key_tmp(tfhe_context* ctx, const u32* host, size_t words, size_t at) {
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_key_tmp.as<u32>() + at, host, words * sizeof(u32), hipMemcpyHostToDevice,
                              ctx->stream));
  return TFHE_OK;
}

// rows of GLWE ciphertexts [rows][k+1][N] on the device; sk already at d_key_tmp[0 .. kN)
int glwe_rows_add_mask_dot_key(tfhe_context* ctx, u32* d_rows, size_t rows) {
  const u32 k = ctx->params.glwe_dimension;
  HIP_TRY(ctx, launch::glwe_body(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->d_tw.as(), k, d_rows, rows,
                                 ctx->d_key_tmp.as<u32>(), d_rows + (size_t)k * ctx->N,
                                 (size_t)(k + 1) * ctx->N, false));
  return TFHE_OK;
}

// generate_ksk (key_switching.rs:20-60) on device rows; both keys are host pointers
int ksk_gen_device(tfhe_context* ctx, const u32* from_sk, size_t from_dim, const u32* to_sk,
                   size_t to_dim, u32* d_ksk) {
  const std::vector<u32> factor = gadget_factors(ctx, from_sk, from_dim);  // in the rows' b slots
  const size_t rows = factor.size();
  TFHE_TRY(ensure_key_tmp(ctx, to_dim + rows));
  TFHE_TRY(to_key_tmp(ctx, to_sk, to_dim, 0));
  TFHE_TRY(to_key_tmp(ctx, factor.data(), rows, to_dim));
  HIP_TRY(ctx, launch::lwe_body(ctx->stream, d_ksk, rows, (u32)to_dim, ctx->d_key_tmp.as<u32>(),
                                ctx->d_key_tmp.as<u32>() + to_dim, d_ksk + to_dim, to_dim + 1, false));
  // `factor` is pageable host memory: the async copy has staged it before returning
  return TFHE_OK;
}

}  // namespace

int tfhe_glwe_encrypt_zero_batch_device(tfhe_context* ctx, const uint32_t* glwe_sk, uint32_t* glwe,
                                        size_t count) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe_sk, glwe}, count));
  const size_t kn = ctx->big_n;
  TFHE_TRY(check_binary(ctx, glwe_sk, kn, "glwe secret key"));
  TFHE_TRY(ensure_key_tmp(ctx, kn));
  TFHE_TRY(to_key_tmp(ctx, glwe_sk, kn, 0));
  return glwe_rows_add_mask_dot_key(ctx, glwe, count);
}

int tfhe_glwe_encrypt_zero_batch(tfhe_context* ctx, const uint32_t* glwe_sk, uint32_t* glwe, size_t count) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe_sk, glwe}, count));
  return in_place_host_form(ctx, glwe, count * glwe_words(ctx),
                            [&](u32* d) { return tfhe_glwe_encrypt_zero_batch_device(ctx, glwe_sk, d, count); });
}

int tfhe_glwe_decrypt_batch(tfhe_context* ctx, const uint32_t* glwe_sk, const uint32_t* glwe, size_t count,
                            uint32_t* plaintext_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe_sk, glwe, plaintext_out}, count));
  const u32 k = ctx->params.glwe_dimension;
  const size_t kn = ctx->big_n;
  TFHE_TRY(check_binary(ctx, glwe_sk, kn, "glwe secret key"));
  TFHE_TRY(ensure_key_tmp(ctx, kn));
  enum { kIn, kOut };
  Staging s(ctx, {count * glwe_words(ctx), count * ctx->N});
  TFHE_TRY(s.reserve());
  TFHE_TRY(to_key_tmp(ctx, glwe_sk, kn, 0));
  TFHE_TRY(s.upload(kIn, glwe));
  HIP_TRY(ctx, launch::glwe_body(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->d_tw.as(), k, s[kIn], count,
                                 ctx->d_key_tmp.as<u32>(), s[kOut], ctx->N, true));
  return s.download_and_wait(kOut, plaintext_out);
}

int tfhe_ggsw_encrypt_batch_device(tfhe_context* ctx, const uint32_t* glwe_sk, const uint32_t* messages,
                                   uint32_t* ggsw, size_t count) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe_sk, messages, ggsw}, count));
  const u32 k = ctx->params.glwe_dimension;
  const size_t kn = ctx->big_n;
  TFHE_TRY(check_binary(ctx, glwe_sk, kn, "glwe secret key"));
  TFHE_TRY(ensure_key_tmp(ctx, kn + count));
  TFHE_TRY(to_key_tmp(ctx, glwe_sk, kn, 0));
  TFHE_TRY(to_key_tmp(ctx, messages, count, kn));
  TFHE_TRY(glwe_rows_add_mask_dot_key(ctx, ggsw, count * ctx->R));
  HIP_TRY(ctx, launch::ggsw_add_gadget(ctx->stream, ggsw, count, k, ctx->pbs.log_n, ctx->pbs.levels,
                                       ctx->pbs.log_base, gadget_top(ctx, ctx->pbs.log_base),
                                       ctx->d_key_tmp.as<u32>() + kn));
  return TFHE_OK;
}

int tfhe_ggsw_encrypt_batch(tfhe_context* ctx, const uint32_t* glwe_sk, const uint32_t* messages,
                            uint32_t* ggsw, size_t count) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {glwe_sk, messages, ggsw}, count));
  return in_place_host_form(ctx, ggsw, count * ggsw_words(ctx),
                            [&](u32* d) { return tfhe_ggsw_encrypt_batch_device(ctx, glwe_sk, messages, d, count); });
}

int tfhe_lwe_encrypt_batch_device(tfhe_context* ctx, const uint32_t* lwe_sk, size_t dimension,
                                  const uint32_t* plaintexts, uint32_t* lwe, size_t batch) {
  TFHE_TRY(check_ctx(ctx));
  if (!lwe_sk || !lwe || batch == 0 || dimension == 0 || dimension >= (1u << 31))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer / empty batch / bad dimension");
  TFHE_TRY(check_binary(ctx, lwe_sk, dimension, "lwe secret key"));
  TFHE_TRY(ensure_key_tmp(ctx, dimension));
  TFHE_TRY(to_key_tmp(ctx, lwe_sk, dimension, 0));
  HIP_TRY(ctx, launch::lwe_body(ctx->stream, lwe, batch, (u32)dimension, ctx->d_key_tmp.as<u32>(), plaintexts,
                                lwe + dimension, dimension + 1, false));
  return TFHE_OK;
}

int tfhe_lwe_encrypt_batch(tfhe_context* ctx, const uint32_t* lwe_sk, size_t dimension,
                           const uint32_t* plaintexts, uint32_t* lwe, size_t batch) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {lwe_sk, lwe}, batch && dimension));
  enum { kLwe, kPlaintexts };
  Staging s(ctx, {batch * (dimension + 1), batch});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kLwe, lwe));
  if (plaintexts) TFHE_TRY(s.upload(kPlaintexts, plaintexts));
  TFHE_TRY(tfhe_lwe_encrypt_batch_device(ctx, lwe_sk, dimension, plaintexts ? s[kPlaintexts] : nullptr, s[kLwe], batch));
  return s.download_and_wait(kLwe, lwe);
}

int tfhe_lwe_decrypt_batch_device(tfhe_context* ctx, const uint32_t* lwe_sk, size_t dimension,
                                  const uint32_t* lwe, size_t batch, uint32_t* plaintext_out) {
  TFHE_TRY(check_ctx(ctx));
  if (!lwe_sk || !lwe || !plaintext_out || batch == 0 || dimension == 0 || dimension >= (1u << 31))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer / empty batch / bad dimension");
  TFHE_TRY(check_binary(ctx, lwe_sk, dimension, "lwe secret key"));
  TFHE_TRY(ensure_key_tmp(ctx, dimension));
  TFHE_TRY(to_key_tmp(ctx, lwe_sk, dimension, 0));
  HIP_TRY(ctx, launch::lwe_body(ctx->stream, lwe, batch, (u32)dimension, ctx->d_key_tmp.as<u32>(), nullptr,
                                plaintext_out, 1, true));
  return TFHE_OK;
}

int tfhe_lwe_decrypt_batch(tfhe_context* ctx, const uint32_t* lwe_sk, size_t dimension, const uint32_t* lwe,
                           size_t batch, uint32_t* plaintext_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {lwe_sk, lwe, plaintext_out}, batch && dimension));
  enum { kLwe, kOut };
  Staging s(ctx, {batch * (dimension + 1), batch});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kLwe, lwe));
  TFHE_TRY(tfhe_lwe_decrypt_batch_device(ctx, lwe_sk, dimension, s[kLwe], batch, s[kOut]));
  return s.download_and_wait(kOut, plaintext_out);
}

int tfhe_generate_ksk(tfhe_context* ctx, const uint32_t* from_sk, size_t from_dimension,
                      const uint32_t* to_sk, size_t to_dimension, uint32_t* ksk) {
  TFHE_TRY(check_ctx(ctx));
  if (!from_sk || !to_sk || !ksk || from_dimension == 0 || to_dimension == 0 || to_dimension >= (1u << 31))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer / bad dimension");
  TFHE_TRY(check_binary(ctx, from_sk, from_dimension, "from secret key"));
  TFHE_TRY(check_binary(ctx, to_sk, to_dimension, "to secret key"));
  return in_place_host_form(ctx, ksk, from_dimension * ctx->ks.levels * (to_dimension + 1),
                            [&](u32* d) { return ksk_gen_device(ctx, from_sk, from_dimension, to_sk, to_dimension, d); });
}

// notes/BMMP Bootstrapping.md:22-24: the three GGSW messages of key-bit pair j
static std::vector<u32> bmmp_messages(const u32* lwe_sk, size_t n) {
  std::vector<u32> m(n / 2 * 3);
  for (size_t j = 0; j < n / 2; ++j) {
    const u32 s0 = lwe_sk[2 * j], s1 = lwe_sk[2 * j + 1];
    m[3 * j + 0] = s0 * s1;
    m[3 * j + 1] = s0 * (1u - s1);
    m[3 * j + 2] = s1 * (1u - s0);
  }
  return m;
}

// bootstrapping_key_gen: a GGSW per key bit (bootstrapping.rs:32-38) -- per message of a pair of key bits with bmmp --
// and the key-switching key from the flattened GLWE key to the LWE key (:41-51, lwe.rs:62-73)
static int key_gen_device(tfhe_context* ctx, const u32* lwe_sk, const u32* glwe_sk, u32* bsk, u32* ksk, int load, bool bmmp) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {lwe_sk, glwe_sk, bsk, ksk}, 1, "null pointer"));
  if (bmmp) TFHE_TRY(check_bmmp(ctx));
  const size_t n = ctx->params.lwe_dimension;
  TFHE_TRY(check_binary(ctx, lwe_sk, n, "lwe secret key"));
  const std::vector<u32> messages = bmmp ? bmmp_messages(lwe_sk, n) : std::vector<u32>(lwe_sk, lwe_sk + n);
  TFHE_TRY(tfhe_ggsw_encrypt_batch_device(ctx, glwe_sk, messages.data(), bsk, messages.size()));
  TFHE_TRY(ksk_gen_device(ctx, glwe_sk, ctx->big_n, lwe_sk, n, ksk));
  // `messages` is pageable host memory: the async copy inside has staged it before returning
  if (load) return load_key_common(ctx, bsk, ksk, true, bmmp);
  return TFHE_OK;
}

static int key_gen_host(tfhe_context* ctx, const u32* lwe_sk, const u32* glwe_sk, u32* bsk, u32* ksk, int load, bool bmmp) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {lwe_sk, glwe_sk, bsk, ksk}, 1, "null pointer"));
  if (bmmp) TFHE_TRY(check_bmmp(ctx));
  const size_t bsk_bytes = key_ggsws(ctx, bmmp) * ggsw_words(ctx) * sizeof(u32), ksk_bytes = ksk_words(ctx) * sizeof(u32);
  DeviceBuffer d_bsk, d_ksk;
  TFHE_TRY(d_bsk.grow(ctx, bsk_bytes));
  TFHE_TRY(d_ksk.grow(ctx, ksk_bytes));
  hipError_t e = hipMemcpy(d_bsk.as(), bsk, bsk_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_ksk.as(), ksk, ksk_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(ctx, e, "key buffers");
  TFHE_TRY(key_gen_device(ctx, lwe_sk, glwe_sk, d_bsk.as<u32>(), d_ksk.as<u32>(), load, bmmp));
  e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(bsk, d_bsk.as(), bsk_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ksk, d_ksk.as(), ksk_bytes, hipMemcpyDeviceToHost);
  return e == hipSuccess ? TFHE_OK : hip_fail(ctx, e, "key download");
}

int tfhe_bootstrapping_key_gen_device(tfhe_context* ctx, const uint32_t* lwe_sk, const uint32_t* glwe_sk,
                                      uint32_t* bsk, uint32_t* ksk, int load) {
  return key_gen_device(ctx, lwe_sk, glwe_sk, bsk, ksk, load, false);
}

int tfhe_bootstrapping_key_gen(tfhe_context* ctx, const uint32_t* lwe_sk, const uint32_t* glwe_sk,
                               uint32_t* bsk, uint32_t* ksk, int load) {
  return key_gen_host(ctx, lwe_sk, glwe_sk, bsk, ksk, load, false);
}

int tfhe_bootstrapping_key_gen_bmmp_device(tfhe_context* ctx, const uint32_t* lwe_sk, const uint32_t* glwe_sk,
                                           uint32_t* bsk_bmmp, uint32_t* ksk, int load) {
  return key_gen_device(ctx, lwe_sk, glwe_sk, bsk_bmmp, ksk, load, true);
}

int tfhe_bootstrapping_key_gen_bmmp(tfhe_context* ctx, const uint32_t* lwe_sk, const uint32_t* glwe_sk,
                                    uint32_t* bsk_bmmp, uint32_t* ksk, int load) {
  return key_gen_host(ctx, lwe_sk, glwe_sk, bsk_bmmp, ksk, load, true);
}

// ---------------------------------------------------------------------------------- packing key switch
namespace {

// transposed inputs of one launch pair of a packing call: as many outputs as fit 64 MiB (cfg2: 24 of 2.6 MB), at
// least one.  Sized at key load, so that tfhe_pack_lwe_batch_device never allocates.
constexpr size_t kPackColsWords = (size_t)16 << 20;

size_t pack_cols_words_per_group(const tfhe_context* ctx) { return (ctx->pksk_dim + 1) * (size_t)ctx->N; }

// Why this backend cannot pack under the context's KS decomposer, or "" if it can.  A packing call sums the
// R_c = (k+1) l_ks rows of one slice in the transform domain and nothing more (pbs_wave.h::pack_lwe_team), so the bounds
// are the external product's with R_c rows and the KS base.
std::string packing_refusal(const tfhe_context* ctx) {
  return exactness_refusal(ctx, (int)((ctx->params.glwe_dimension + 1) * ctx->ks.levels), (int)ctx->ks.log_base,
                           {"KS log_base", "(k+1) l_ks", "slice"});
}

// d_raw: [from_dimension * l_ks][k+1][N] on the device
int load_packing_key_common(tfhe_context* ctx, const u32* d_raw, size_t from_dimension) {
  const std::string why = packing_refusal(ctx);
  if (!why.empty()) return fail(ctx, TFHE_ERR_EXACTNESS, "packing key refused: " + why);
  const u32 k1 = ctx->params.glwe_dimension + 1;
  const size_t slices = (from_dimension + k1 - 1) / k1;
  const size_t poly_bytes = (size_t)ctx->parts * ctx->N * sizeof(u64);  // one prepared key polynomial
  const size_t polys = from_dimension * ctx->ks.levels * k1;
  const size_t bytes = slices * k1 * ctx->ks.levels * k1 * poly_bytes;
  // until the new key is complete the context holds none
  ctx->have_pksk = false;
  TFHE_TRY(ctx->d_pksk.resize(ctx, bytes));
  ctx->pksk_dim = from_dimension;
  TFHE_TRY(ctx->d_pack_cols.grow(ctx, std::max(kPackColsWords, pack_cols_words_per_group(ctx)) * sizeof(u32)));
  // rows past from_dimension (the last slice, when k+1 does not divide it): zero spectra
  if (polys * poly_bytes < bytes)
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_pksk.as<unsigned char>() + polys * poly_bytes, 0, bytes - polys * poly_bytes, ctx->stream));
  HIP_TRY(ctx, launch::bsk_prepare(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->pbs.k, ctx->d_tw.as(), d_raw, polys, ctx->d_pksk.as()));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->have_pksk = true;
  return TFHE_OK;
}

int check_packing_dimension(tfhe_context* ctx, size_t from_dimension) {
  if (from_dimension == 0 || from_dimension >= (1u << 24))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "from_dimension must be in [1, 2^24)");
  return TFHE_OK;
}

int check_packing_key_args(tfhe_context* ctx, std::initializer_list<const void*> ptrs, const char* null_text, size_t from_dimension) {
  TFHE_TRY(check_present(ctx, ptrs, 1, null_text));
  return check_packing_dimension(ctx, from_dimension);
}

// glwe_out [groups][k+1][N] = Pack of lwe_in [groups][per_group][pksk_dim + 1], input j on coefficients
// [j << log_rep, (j+1) << log_rep): a memset (a memset node under stream capture; the teams add their partial sums into
// the output), then a transpose and a packing launch per chunk of groups the transposed-input workspace holds
int enqueue_pack(tfhe_context* ctx, const u32* lwe_in, size_t groups, u32 per_group, u32* glwe_out, u32 log_rep = 0) {
  const u32 d = (u32)ctx->pksk_dim;
  const size_t glwe = glwe_words(ctx);
  const PbsParams P = packing_params(ctx);
  HIP_TRY(ctx, hipMemsetAsync(glwe_out, 0, groups * glwe * sizeof(u32), ctx->stream));
  const size_t chunk = ctx->d_pack_cols.words() / pack_cols_words_per_group(ctx);  // >= 1 by construction
  for (size_t g0 = 0; g0 < groups; g0 += chunk) {
    const size_t here = std::min(chunk, groups - g0);
    HIP_TRY(ctx, launch::pack_transpose(ctx->stream, lwe_in + g0 * per_group * ((size_t)d + 1), here, per_group, d,
                                        ctx->pbs.log_n, ctx->d_pack_cols.as<u32>(), log_rep));
    HIP_TRY(ctx, launch::pack_lwe(ctx->stream, ctx->field, P, ctx->d_tw.as(), ctx->d_pksk.as(), ctx->d_pack_cols.as<u32>(), d, here,
                                  glwe_out + g0 * glwe));
  }
  return TFHE_OK;
}

}  // namespace

int tfhe_generate_packing_key_device(tfhe_context* ctx, const uint32_t* from_sk, size_t from_dimension,
                                     const uint32_t* glwe_sk, uint32_t* pksk) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_packing_key_args(ctx, {from_sk, glwe_sk, pksk}, "null pointer", from_dimension));
  const size_t kn = ctx->big_n;
  TFHE_TRY(check_binary(ctx, from_sk, from_dimension, "from secret key"));
  TFHE_TRY(check_binary(ctx, glwe_sk, kn, "glwe secret key"));
  // row i*levels + level is a zero encryption plus s_i g_level on coefficient 0 of the body
  const std::vector<u32> factor = gadget_factors(ctx, from_sk, from_dimension);
  const size_t rows = factor.size();
  TFHE_TRY(ensure_key_tmp(ctx, kn + rows));
  TFHE_TRY(to_key_tmp(ctx, glwe_sk, kn, 0));
  TFHE_TRY(to_key_tmp(ctx, factor.data(), rows, kn));
  TFHE_TRY(glwe_rows_add_mask_dot_key(ctx, pksk, rows));
  HIP_TRY(ctx, launch::packing_add_gadget(ctx->stream, pksk, rows, ctx->params.glwe_dimension, ctx->pbs.log_n, ctx->d_key_tmp.as<u32>() + kn));
  // `factor` is pageable host memory: the async copy has staged it before returning
  return TFHE_OK;
}

int tfhe_generate_packing_key(tfhe_context* ctx, const uint32_t* from_sk, size_t from_dimension,
                              const uint32_t* glwe_sk, uint32_t* pksk) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_packing_key_args(ctx, {from_sk, glwe_sk, pksk}, "null pointer", from_dimension));
  return in_place_host_form(ctx, pksk, packing_key_words(ctx, from_dimension), [&](u32* d) {
    return tfhe_generate_packing_key_device(ctx, from_sk, from_dimension, glwe_sk, d);
  });
}

int tfhe_load_packing_key_device(tfhe_context* ctx, const uint32_t* pksk, size_t from_dimension) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_packing_key_args(ctx, {pksk}, "null key pointer", from_dimension));
  return load_packing_key_common(ctx, pksk, from_dimension);
}

int tfhe_load_packing_key(tfhe_context* ctx, const uint32_t* pksk, size_t from_dimension) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_packing_key_args(ctx, {pksk}, "null key pointer", from_dimension));
  const std::string why = packing_refusal(ctx);  // before the upload
  if (!why.empty()) return fail(ctx, TFHE_ERR_EXACTNESS, "packing key refused: " + why);
  const size_t words = packing_key_words(ctx, from_dimension);
  DeviceBuffer raw;
  TFHE_TRY(raw.grow(ctx, words * sizeof(u32)));
  HIP_TRY(ctx, hipMemcpy(raw.as(), pksk, words * sizeof(u32), hipMemcpyHostToDevice));
  return load_packing_key_common(ctx, raw.as<u32>(), from_dimension);
}

int tfhe_packing_key_dimension(const tfhe_context* ctx, size_t* from_dimension) {
  if (!ctx || !from_dimension) return TFHE_ERR_INVALID_ARGUMENT;
  if (!ctx->have_pksk) return TFHE_ERR_NO_KEY;
  *from_dimension = ctx->pksk_dim;
  return TFHE_OK;
}

static int check_pack_args(tfhe_context* ctx, const void* in, size_t groups, size_t per_group, const void* out) {
  TFHE_TRY(check_present(ctx, {in, out}, 1, "null pointer"));
  if (groups == 0 || groups > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "groups must be in [1, 2^31)");
  if (per_group == 0 || per_group > ctx->N)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "per_group must be in [1, N]: a GLWE has N coefficients");
  if (!ctx->have_pksk) return fail(ctx, TFHE_ERR_NO_KEY, "load a packing key first (tfhe_load_packing_key)");
  return TFHE_OK;
}

int tfhe_pack_lwe_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t groups, size_t per_group,
                               uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_pack_args(ctx, lwe_in, groups, per_group, glwe_out));
  return enqueue_pack(ctx, lwe_in, groups, (u32)per_group, glwe_out);
}

int tfhe_pack_lwe_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t groups, size_t per_group,
                        uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_pack_args(ctx, lwe_in, groups, per_group, glwe_out));
  enum { kIn, kOut };
  Staging s(ctx, {groups * per_group * (ctx->pksk_dim + 1), groups * glwe_words(ctx)});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, lwe_in));
  TFHE_TRY(tfhe_pack_lwe_batch_device(ctx, s[kIn], groups, per_group, s[kOut]));
  return s.download_and_wait(kOut, glwe_out);
}

// ---------------------------------------------------------------------------------- GLWE key switch / automorphism
// tfhe_hip.h states the operation, glwe_switch.h::glwe_switch_team the team's work.  A switch key is ONE packing slice of
// dimension k, so it is admitted exactly where a packing key is (packing_refusal) and prepared the same way.
namespace {

int check_switch_key_gen(tfhe_context* ctx, const int32_t* from_polys, const u32* glwe_sk, const u32* key) {
  TFHE_TRY(check_present(ctx, {from_polys, glwe_sk, key}, 1, "null pointer"));
  const size_t kn = ctx->big_n;
  for (size_t i = 0; i < kn; ++i)
    if (from_polys[i] < -1 || from_polys[i] > 1)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "from_polys must have coefficients in {-1, 0, 1}");
  return check_binary(ctx, glwe_sk, kn, "glwe secret key");
}

int switch_key_refusal(tfhe_context* ctx) {
  const std::string why = packing_refusal(ctx);
  if (!why.empty()) return fail(ctx, TFHE_ERR_EXACTNESS, "GLWE switch key refused: " + why);
  return TFHE_OK;
}

// d_raw: [k l_ks][k+1][N] on the device
int prepare_switch_key_common(tfhe_context* ctx, const u32* d_raw, tfhe_glwe_switch_key** out) {
  const u32 k = ctx->params.glwe_dimension, k1 = k + 1;
  const size_t poly_bytes = (size_t)ctx->parts * ctx->N * sizeof(u64);  // one prepared key polynomial
  const size_t polys = (size_t)k * ctx->ks.levels * k1;
  const size_t bytes = (size_t)k1 * ctx->ks.levels * k1 * poly_bytes;
  tfhe_glwe_switch_key* h = new (std::nothrow) tfhe_glwe_switch_key();
  if (!h) return fail(ctx, TFHE_ERR_HIP, "out of host memory");
  h->owner = ctx;
  h->device = ctx->device;
  h->field = ctx->field;
  h->log_n = ctx->pbs.log_n;
  h->k = k;
  h->levels = ctx->ks.levels;
  int st = h->d_key.grow(ctx, bytes);
  if (st == TFHE_OK) {
    // polynomial k of the slice reads zeros against zero key rows: the packing slice's own padding
    hipError_t e = hipMemsetAsync(h->d_key.as<unsigned char>() + polys * poly_bytes, 0, bytes - polys * poly_bytes, ctx->stream);
    if (e == hipSuccess)
      e = launch::bsk_prepare(ctx->stream, ctx->field, ctx->pbs.log_n, ctx->pbs.k, ctx->d_tw.as(), d_raw, polys, h->d_key.as());
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's raw key is free again on return
    if (e != hipSuccess) st = hip_fail(ctx, e, "tfhe_prepare_glwe_switch_key");
  }
  if (st != TFHE_OK) {
    tfhe_glwe_switch_key_destroy(h);
    return st;
  }
  *out = h;
  return TFHE_OK;
}

// t odd in [1, 2N) -> t^-1 mod 2N (Newton's iteration on the 2-adic inverse: five steps give 32 bits)
int automorphism_inverse(tfhe_context* ctx, size_t t, u32* t_inv) {
  if (!(t & 1u) || t >= 2 * (size_t)ctx->N)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "t must be odd and below 2N: X -> X^t is a ring automorphism only then");
  u32 u = (u32)t;
  for (int i = 0; i < 5; ++i) u *= 2u - (u32)t * u;
  *t_inv = u & (2u * ctx->N - 1u);
  return TFHE_OK;
}

int check_automorphism_args(tfhe_context* ctx, const u32* in, size_t batch, size_t t, const tfhe_glwe_switch_key* key,
                            const u32* out, u32* t_inv) {
  TFHE_TRY(check_present(ctx, {in, out}, 1, "null pointer"));
  if (batch == 0 || batch > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch must be in [1, 2^31)");
  TFHE_TRY(automorphism_inverse(ctx, t, t_inv));
  if (key && (key->owner != ctx || key->device != ctx->device || key->field != ctx->field || key->log_n != ctx->pbs.log_n ||
              key->k != ctx->params.glwe_dimension || key->levels != ctx->ks.levels || !key->d_key))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the switch key was prepared by another context or backend");
  const size_t words = batch * glwe_words(ctx);
  if (in != out && overlap(in, words, out, words))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "glwe_out overlaps glwe_in without being it: in place means the same pointer");
  return TFHE_OK;
}

}  // namespace

int tfhe_glwe_sk_automorphism(const uint32_t* glwe_sk, size_t k, unsigned log_n, size_t t, int32_t* out) {
  if (!glwe_sk || !out || k == 0 || log_n == 0 || log_n > 30) return TFHE_ERR_INVALID_ARGUMENT;
  const size_t N = (size_t)1 << log_n;
  if (!(t & 1u) || t >= 2 * N) return TFHE_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < k * N; ++i)
    if (glwe_sk[i] > 1u) return TFHE_ERR_INVALID_ARGUMENT;
  for (size_t p = 0; p < k; ++p)
    for (size_t j = 0; j < N; ++j) {  // coefficient j lands on j t mod N, negated when j t mod 2N >= N
      const size_t at = (j * t) & (2 * N - 1);
      const int32_t s = (int32_t)glwe_sk[p * N + j];
      out[p * N + (at & (N - 1))] = at >= N ? -s : s;
    }
  return TFHE_OK;
}

int tfhe_generate_glwe_switch_key_device(tfhe_context* ctx, const int32_t* from_polys, const uint32_t* glwe_sk, uint32_t* key) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_switch_key_gen(ctx, from_polys, glwe_sk, key));
  const size_t kn = ctx->big_n;
  const size_t rows = (size_t)ctx->params.glwe_dimension * ctx->ks.levels;
  // row i*levels + level is a zero encryption plus from_polys[i] g_level on the body
  TFHE_TRY(ensure_key_tmp(ctx, 2 * kn));
  TFHE_TRY(to_key_tmp(ctx, glwe_sk, kn, 0));
  TFHE_TRY(to_key_tmp(ctx, reinterpret_cast<const u32*>(from_polys), kn, kn));
  TFHE_TRY(glwe_rows_add_mask_dot_key(ctx, key, rows));
  HIP_TRY(ctx, launch::glwe_switch_add_gadget(ctx->stream, key, ctx->params.glwe_dimension, ctx->pbs.log_n, ctx->ks.levels,
                                              ctx->ks.log_base, gadget_top(ctx, ctx->ks.log_base),
                                              reinterpret_cast<const i32*>(ctx->d_key_tmp.as<u32>() + kn)));
  // the host arrays are pageable memory: the async copies have staged them before returning
  return TFHE_OK;
}

int tfhe_generate_glwe_switch_key(tfhe_context* ctx, const int32_t* from_polys, const uint32_t* glwe_sk, uint32_t* key) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_switch_key_gen(ctx, from_polys, glwe_sk, key));
  return in_place_host_form(ctx, key, glwe_switch_key_words(ctx), [&](u32* d) {
    return tfhe_generate_glwe_switch_key_device(ctx, from_polys, glwe_sk, d);
  });
}

int tfhe_prepare_glwe_switch_key_device(tfhe_context* ctx, const uint32_t* key, tfhe_glwe_switch_key** out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {key, out}, 1, "null pointer"));
  *out = nullptr;
  TFHE_TRY(switch_key_refusal(ctx));
  return prepare_switch_key_common(ctx, key, out);
}

int tfhe_prepare_glwe_switch_key(tfhe_context* ctx, const uint32_t* key, tfhe_glwe_switch_key** out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {key, out}, 1, "null pointer"));
  *out = nullptr;
  TFHE_TRY(switch_key_refusal(ctx));  // before the upload
  const size_t words = glwe_switch_key_words(ctx);
  DeviceBuffer raw;
  TFHE_TRY(raw.grow(ctx, words * sizeof(u32)));
  HIP_TRY(ctx, hipMemcpy(raw.as(), key, words * sizeof(u32), hipMemcpyHostToDevice));
  return prepare_switch_key_common(ctx, raw.as<u32>(), out);
}

void tfhe_glwe_switch_key_destroy(tfhe_glwe_switch_key* key) {
  if (!key) return;
  (void)hipSetDevice(key->device);  // before `delete` releases the spectra
  delete key;
}

int tfhe_glwe_automorphism_batch_device(tfhe_context* ctx, const uint32_t* glwe_in, size_t batch, size_t t,
                                        const tfhe_glwe_switch_key* key, int add_input, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  u32 t_inv = 0;
  TFHE_TRY(check_automorphism_args(ctx, glwe_in, batch, t, key, glwe_out, &t_inv));
  if (!key) {
    if (add_input)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "add_input needs a key: without one the result is under another key than the input");
    HIP_TRY(ctx, launch::glwe_automorphism(ctx->stream, glwe_in, batch * (ctx->params.glwe_dimension + 1), ctx->pbs.log_n, t_inv, glwe_out));
    return TFHE_OK;
  }
  HIP_TRY(ctx, launch::glwe_switch(ctx->stream, ctx->field, packing_params(ctx), ctx->d_tw.as(), key->d_key.as(), glwe_in, batch,
                                   t_inv, add_input != 0, glwe_out));
  return TFHE_OK;
}

int tfhe_glwe_automorphism_batch(tfhe_context* ctx, const uint32_t* glwe_in, size_t batch, size_t t,
                                 const tfhe_glwe_switch_key* key, int add_input, uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  u32 t_inv = 0;
  TFHE_TRY(check_automorphism_args(ctx, glwe_in, batch, t, key, glwe_out, &t_inv));
  const size_t words = batch * glwe_words(ctx);
  Staging s(ctx, {words});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(0, glwe_in));
  TFHE_TRY(tfhe_glwe_automorphism_batch_device(ctx, s[0], batch, t, key, add_input, s[0]));  // in place
  return s.download_and_wait(0, glwe_out);
}

// ---------------------------------------------------------------------------------- multi-bit blind rotation
// tfhe_hip.h states the operation, multibit.h the two launches: the bundles of a call -- one prepared GGSW per (sample,
// group of g key bits) -- go to the reserved workspace, the wide team then rotates over them.
namespace {

int check_multibit_bits(tfhe_context* ctx, unsigned g) {
  if (g < 2 || g > (unsigned)kMultibitMaxBits)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "g must be 2, 3 or 4 key bits per group, got " + std::to_string(g));
  return TFHE_OK;
}

// the multi-bit rotation runs on the wide team: refused wherever the launcher does not offer that shape
int multibit_refusal(tfhe_context* ctx) {
  int why = 0;
  if (launch::multibit_refusal(ctx->field, ctx->pbs, &why) != hipSuccess) why = launch::kMultibitNoRing;
  const std::string head = "the multi-bit blind rotation runs on the wide team, which is offered ";
  switch (why) {
    case 0: return TFHE_OK;
    case launch::kMultibitNoBackend:
      return fail(ctx, TFHE_ERR_UNSUPPORTED, head + "in the fp64-fft backend only; this context uses " + tfhe_context_backend(ctx));
    case launch::kMultibitNoLds:
      return fail(ctx, TFHE_ERR_UNSUPPORTED, head + "while its (k+1) l = " + std::to_string(ctx->R) +
                                                 " row buffers fit the 160 KiB of LDS of a CU; these parameters need more");
    default:
      return fail(ctx, TFHE_ERR_UNSUPPORTED, head + "up to N = 1024; this context has N = " + std::to_string(ctx->N));
  }
}

int check_multibit_key(tfhe_context* ctx, const tfhe_multibit_key* key) {
  if (!key) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer");
  if (key->owner != ctx || key->device != ctx->device || !key->d_key || key->groups != multibit_groups(ctx, key->g))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the multi-bit key was prepared by another context");
  return TFHE_OK;
}

int check_multibit_batch(tfhe_context* ctx, size_t batch, size_t count, const char* count_name) {
  if (batch == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "empty batch");
  if (batch > 65535) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch exceeds 65535 (the bundle launch's second grid dimension)");
  if (count != 1 && count != batch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, std::string(count_name) + " must be 1 or batch");
  return TFHE_OK;
}

int check_multibit_reserved(tfhe_context* ctx, const tfhe_multibit_key* key, size_t batch) {
  const size_t need = multibit_bundle_bytes(ctx, batch, key->g);
  if (need > ctx->d_mb_ws.bytes() || batch > ctx->ws_batch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the bundles of " + std::to_string(batch) + " samples at g = " + std::to_string(key->g) + " need " + std::to_string(need) +
                    " bytes, reserved " + std::to_string(ctx->d_mb_ws.bytes()) + ": call tfhe_context_reserve_multibit(ctx, " +
                    std::to_string(batch) + ", " + std::to_string(key->g) + ") first");
  return TFHE_OK;
}

int reserve_multibit(tfhe_context* ctx, size_t batch, unsigned g) {
  TFHE_TRY(reserve(ctx, batch));
  return ctx->d_mb_ws.grow(ctx, multibit_bundle_bytes(ctx, batch, g));
}

// what a rotation starts from: clear test vectors [tv_count][N], or GLWE accumulators [tv_count][k+1][N] and an offset
struct MultibitSource {
  const u32* acc;
  size_t count;
  bool glwe;
  u32 offset;
};

hipError_t enqueue_multibit_rotate(tfhe_context* ctx, const tfhe_multibit_key* key, const u32* lwe_in, size_t batch, const MultibitSource& from,
                                   u32* glwe_out, u32* lwe_extracted, bool time_launches = false) {
  PbsParams P = ctx->pbs;
  P.acc_glwe = from.glwe ? 1u : 0u;
  P.acc_offset = from.offset;
  const size_t words = from.glwe ? glwe_words(ctx) : (size_t)ctx->N;
  auto mark = [&](int i) { return time_launches && ctx->timing ? hipEventRecord(ctx->ev[i], ctx->stream) : hipSuccess; };
  hipError_t e = mark(0);
  if (e == hipSuccess)
    e = launch::multibit_bundle(ctx->stream, ctx->field, P, ctx->d_tw.as(), key->d_key.as<u32>(), key->g, lwe_in, batch, ctx->d_mb_ws.as());
  if (e == hipSuccess) e = mark(1);
  if (e == hipSuccess) e = mark(2);
  if (e == hipSuccess)
    e = launch::multibit_rotate(ctx->stream, ctx->field, P, ctx->d_tw.as(), lwe_in, batch, from.acc, from.count == 1 ? 0 : words,
                                ctx->d_mb_ws.as(), key->groups, glwe_out, lwe_extracted);
  if (e == hipSuccess) e = mark(3);
  return e;
}

int check_multibit_rotate_args(tfhe_context* ctx, const tfhe_multibit_key* key, const void* lwe_in, size_t batch, const void* tv,
                               size_t tv_count, const void* acc_in, size_t rotation_offset, const void* glwe_out, const void* lwe_extracted) {
  TFHE_TRY(check_multibit_key(ctx, key));
  if (!lwe_in) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer");
  if ((tv != nullptr) == (acc_in != nullptr))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "pass either test_vector_poly or acc_in, not both and not neither");
  if (!glwe_out && !lwe_extracted) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "pass glwe_out, lwe_extracted or both");
  TFHE_TRY(check_multibit_batch(ctx, batch, tv_count, acc_in ? "acc_count" : "tv_count"));
  if (acc_in && rotation_offset >= 2 * (size_t)ctx->N)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "rotation_offset must be below 2N = " + std::to_string(2 * (size_t)ctx->N));
  if (!acc_in && rotation_offset != 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "rotation_offset goes with acc_in");
  return TFHE_OK;
}

int check_multibit_bootstrap_args(tfhe_context* ctx, const tfhe_multibit_key* key, const void* lwe_in, size_t batch, const void* tv,
                                  size_t tv_count, const void* lwe_out) {
  TFHE_TRY(check_multibit_key(ctx, key));
  TFHE_TRY(check_present(ctx, {lwe_in, tv, lwe_out}, 1, "null pointer"));
  TFHE_TRY(check_multibit_batch(ctx, batch, tv_count, "tv_count"));
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "load a key-switching key first (tfhe_load_bootstrapping_key carries it)");
  return TFHE_OK;
}

// message of slot (group, p - 1): the group's bits are exactly the pattern p; slots past a ragged group's patterns hold 0
void multibit_messages(const u32* lwe_sk, size_t n, unsigned g, std::vector<u32>* out) {
  const size_t groups = (n + g - 1) / g, slots = ((size_t)1 << g) - 1;
  std::vector<u32>& m = *out;
  m.assign(groups * slots, 0u);
  for (size_t i = 0; i < groups; ++i) {
    const size_t bits = std::min<size_t>(g, n - i * g);
    for (size_t p = 1; p < ((size_t)1 << bits); ++p) {
      u32 v = 1u;
      for (size_t j = 0; j < bits; ++j) v *= ((p >> j) & 1u) ? lwe_sk[i * g + j] : 1u - lwe_sk[i * g + j];
      m[i * slots + p - 1] = v;
    }
  }
}

int check_multibit_key_gen(tfhe_context* ctx, const u32* lwe_sk, const u32* glwe_sk, unsigned g, const u32* bsk_mb) {
  TFHE_TRY(check_present(ctx, {lwe_sk, glwe_sk, bsk_mb}, 1, "null pointer"));
  TFHE_TRY(check_multibit_bits(ctx, g));
  TFHE_TRY(check_binary(ctx, lwe_sk, ctx->params.lwe_dimension, "lwe secret key"));
  return check_binary(ctx, glwe_sk, ctx->big_n, "glwe secret key");
}

int prepare_multibit_key_common(tfhe_context* ctx, const u32* raw, unsigned g, bool raw_on_device, tfhe_multibit_key** out) {
  TFHE_TRY(check_present(ctx, {raw, out}, 1, "null pointer"));
  *out = nullptr;
  TFHE_TRY(check_multibit_bits(ctx, g));
  TFHE_TRY(multibit_refusal(ctx));
  tfhe_multibit_key* h = new (std::nothrow) tfhe_multibit_key();
  if (!h) return fail(ctx, TFHE_ERR_HIP, "out of host memory");
  h->owner = ctx;
  h->device = ctx->device;
  h->g = g;
  h->groups = (u32)multibit_groups(ctx, g);
  const size_t bytes = multibit_key_ggsws(ctx, g) * ggsw_words(ctx) * sizeof(u32);
  int st = h->d_key.grow(ctx, bytes);
  if (st == TFHE_OK) {
    hipError_t e = hipMemcpyAsync(h->d_key.as(), raw, bytes, raw_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's raw key is free again on return
    if (e != hipSuccess) st = hip_fail(ctx, e, "tfhe_prepare_multibit_key");
  }
  if (st != TFHE_OK) {
    tfhe_multibit_key_destroy(h);
    return st;
  }
  *out = h;
  return TFHE_OK;
}

}  // namespace

int tfhe_generate_multibit_key_device(tfhe_context* ctx, const uint32_t* lwe_sk, const uint32_t* glwe_sk, unsigned g, uint32_t* bsk_mb) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_multibit_key_gen(ctx, lwe_sk, glwe_sk, g, bsk_mb));
  std::vector<u32> messages;
  multibit_messages(lwe_sk, ctx->params.lwe_dimension, g, &messages);
  // `messages` is pageable host memory: the async copy inside has staged it before returning
  return tfhe_ggsw_encrypt_batch_device(ctx, glwe_sk, messages.data(), bsk_mb, messages.size());
}

int tfhe_generate_multibit_key(tfhe_context* ctx, const uint32_t* lwe_sk, const uint32_t* glwe_sk, unsigned g, uint32_t* bsk_mb) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_multibit_key_gen(ctx, lwe_sk, glwe_sk, g, bsk_mb));
  return in_place_host_form(ctx, bsk_mb, multibit_key_ggsws(ctx, g) * ggsw_words(ctx),
                            [&](u32* d) { return tfhe_generate_multibit_key_device(ctx, lwe_sk, glwe_sk, g, d); });
}

int tfhe_prepare_multibit_key_device(tfhe_context* ctx, const uint32_t* bsk_mb, unsigned g, tfhe_multibit_key** out) {
  TFHE_TRY(check_ctx(ctx));
  return prepare_multibit_key_common(ctx, bsk_mb, g, true, out);
}

int tfhe_prepare_multibit_key(tfhe_context* ctx, const uint32_t* bsk_mb, unsigned g, tfhe_multibit_key** out) {
  TFHE_TRY(check_ctx(ctx));
  return prepare_multibit_key_common(ctx, bsk_mb, g, false, out);
}

void tfhe_multibit_key_destroy(tfhe_multibit_key* key) {
  if (!key) return;
  (void)hipSetDevice(key->device);  // before `delete` releases the key
  delete key;
}

int tfhe_context_reserve_multibit(tfhe_context* ctx, size_t max_batch, unsigned g) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_multibit_bits(ctx, g));
  TFHE_TRY(check_multibit_batch(ctx, max_batch, 1, "max_batch"));
  TFHE_TRY(multibit_refusal(ctx));
  return reserve_multibit(ctx, max_batch, g);
}

int tfhe_multibit_last_kernel_ms(tfhe_context* ctx, float* bundle_ms, float* rotate_ms) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {bundle_ms, rotate_ms}, 1, "null pointer"));
  if (!ctx->timing || !ctx->ev_valid_mb) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "no timed multi-bit rotation: enable tfhe_context_set_timing first");
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev[3]));
  HIP_TRY(ctx, hipEventElapsedTime(bundle_ms, ctx->ev[0], ctx->ev[1]));
  HIP_TRY(ctx, hipEventElapsedTime(rotate_ms, ctx->ev[2], ctx->ev[3]));
  return TFHE_OK;
}

int tfhe_multibit_blind_rotate_batch_device(tfhe_context* ctx, const tfhe_multibit_key* key, const uint32_t* lwe_in, size_t batch,
                                            const uint32_t* test_vector_poly, size_t tv_count, const uint32_t* acc_in,
                                            size_t rotation_offset, uint32_t* glwe_out, uint32_t* lwe_extracted) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_multibit_rotate_args(ctx, key, lwe_in, batch, test_vector_poly, tv_count, acc_in, rotation_offset, glwe_out, lwe_extracted));
  TFHE_TRY(check_multibit_reserved(ctx, key, batch));
  const MultibitSource from{acc_in ? acc_in : test_vector_poly, tv_count, acc_in != nullptr, (u32)rotation_offset};
  HIP_TRY(ctx, enqueue_multibit_rotate(ctx, key, lwe_in, batch, from, glwe_out, lwe_extracted, true));
  if (ctx->timing) {  // events 0/1 bracket the bundle launch, 2/3 the rotate launch: tfhe_multibit_last_kernel_ms
    ctx->ev_valid_br = ctx->ev_valid_ks = false;
    ctx->ev_valid_mb = true;
  }
  return TFHE_OK;
}

int tfhe_multibit_blind_rotate_batch(tfhe_context* ctx, const tfhe_multibit_key* key, const uint32_t* lwe_in, size_t batch,
                                     const uint32_t* test_vector_poly, size_t tv_count, const uint32_t* acc_in, size_t rotation_offset,
                                     uint32_t* glwe_out, uint32_t* lwe_extracted) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_multibit_rotate_args(ctx, key, lwe_in, batch, test_vector_poly, tv_count, acc_in, rotation_offset, glwe_out, lwe_extracted));
  if (!acc_in) TFHE_TRY(check_tv_host(ctx, test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(reserve_multibit(ctx, batch, key->g));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * lwe_words(ctx)));
  if (acc_in) TFHE_TRY(upload(ctx, ctx->d_glwe_a.as<u32>(), acc_in, tv_count * glwe_words(ctx)));
  else TFHE_TRY(upload(ctx, ctx->d_tv.as<u32>(), test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(tfhe_multibit_blind_rotate_batch_device(ctx, key, ctx->d_lwe_in.as<u32>(), batch, acc_in ? nullptr : ctx->d_tv.as<u32>(), tv_count,
                                                   acc_in ? ctx->d_glwe_a.as<u32>() : nullptr, rotation_offset,
                                                   glwe_out ? ctx->d_glwe_b.as<u32>() : nullptr, lwe_extracted ? ctx->d_lwe_big.as<u32>() : nullptr));
  if (glwe_out) TFHE_TRY(download(ctx, glwe_out, ctx->d_glwe_b.as<u32>(), batch * glwe_words(ctx)));
  if (lwe_extracted) TFHE_TRY(download(ctx, lwe_extracted, ctx->d_lwe_big.as<u32>(), batch * big_lwe_words(ctx)));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_OK;
}

int tfhe_multibit_bootstrap_batch_device(tfhe_context* ctx, const tfhe_multibit_key* key, const uint32_t* lwe_in, size_t batch,
                                         const uint32_t* test_vector_poly, size_t tv_count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_multibit_bootstrap_args(ctx, key, lwe_in, batch, test_vector_poly, tv_count, lwe_out));
  TFHE_TRY(check_multibit_reserved(ctx, key, batch));
  const MultibitSource from{test_vector_poly, tv_count, false, 0u};
  return enqueue_bootstrap_with(ctx, lwe_in, batch, ctx->d_lwe_big.as<u32>(), lwe_out, [&](const u32* br_in, u32* br_out) {
    return enqueue_multibit_rotate(ctx, key, br_in, batch, from, nullptr, br_out);
  });
}

int tfhe_multibit_bootstrap_batch(tfhe_context* ctx, const tfhe_multibit_key* key, const uint32_t* lwe_in, size_t batch,
                                  const uint32_t* test_vector_poly, size_t tv_count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_multibit_bootstrap_args(ctx, key, lwe_in, batch, test_vector_poly, tv_count, lwe_out));
  TFHE_TRY(check_tv_host(ctx, test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(reserve_multibit(ctx, batch, key->g));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * io_words(ctx)));
  TFHE_TRY(upload(ctx, ctx->d_tv.as<u32>(), test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(tfhe_multibit_bootstrap_batch_device(ctx, key, ctx->d_lwe_in.as<u32>(), batch, ctx->d_tv.as<u32>(), tv_count, ctx->d_lwe_out.as<u32>()));
  return download_and_wait(ctx, lwe_out, ctx->d_lwe_out.as<u32>(), batch * io_words(ctx));
}

// ---------------------------------------------------------------------------------- block-binary blind rotation
// tfhe_hip.h states the operation, block_rotate.h the step: `block` key bits per decomposition on the loaded, ordinary
// key.  The workspace is tfhe_context_reserve's: the parked accumulators and the LWE buffers.
namespace {

// the largest block the exactness rule admits (FftField::block_error_bound below kMaxError, b R rows within kMaxRows),
// 0 with the reason where the rotation is not offered
int block_rotate_max_block(tfhe_context* ctx, unsigned* max_block) {
  *max_block = 0;
  const tfhe_params& p = ctx->params;
  if (ctx->field != launch::kFieldFft)
    return fail(ctx, TFHE_ERR_UNSUPPORTED, std::string("the block-binary blind rotation is offered in the fp64-fft backend only; this context uses ") +
                                               tfhe_context_backend(ctx));
  if (!launch::block_rotate_supported(ctx->field, p.glwe_poly_degree, p.glwe_dimension))
    return fail(ctx, TFHE_ERR_UNSUPPORTED, "the block-binary blind rotation is offered with one wave per polynomial, N = 512 and N = 1024; this context has N = " +
                                               std::to_string(ctx->N));
  unsigned b = 1;
  while ((b + 1) * ctx->R <= (unsigned)FftField::kMaxRows &&
         FftField::block_error_bound((int)p.glwe_poly_degree, (int)ctx->R, (int)p.pbs_decomposer.log_base, (int)(b + 1)) < FftField::kMaxError)
    ++b;
  *max_block = b >= 2 ? b : 0;
  if (b < 2) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "fp64-fft: rounding bound %.4g of a block of 2 key bits of %u rows in base 2^%u is not below %.4g",
                  FftField::block_error_bound((int)p.glwe_poly_degree, (int)ctx->R, (int)p.pbs_decomposer.log_base, 2), ctx->R,
                  p.pbs_decomposer.log_base, FftField::kMaxError);
    return fail(ctx, TFHE_ERR_EXACTNESS, buf);
  }
  return TFHE_OK;
}

int check_block(tfhe_context* ctx, unsigned block) {
  if (block < 2) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "block must be at least 2 key bits, got " + std::to_string(block));
  if (ctx->have_key && ctx->bmmp)
    return fail(ctx, TFHE_ERR_UNSUPPORTED, "the block-binary blind rotation needs an ordinary bootstrapping key; a BMMP key is loaded");
  unsigned max_block = 0;
  TFHE_TRY(block_rotate_max_block(ctx, &max_block));
  if (block > max_block) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "fp64-fft: rounding bound %.4g of a block of %u key bits is not below %.4g; the largest admitted block is %u",
                  FftField::block_error_bound((int)ctx->params.glwe_poly_degree, (int)ctx->R, (int)ctx->params.pbs_decomposer.log_base, (int)block),
                  block, FftField::kMaxError, max_block);
    return fail(ctx, TFHE_ERR_EXACTNESS, buf);
  }
  return TFHE_OK;
}

int check_block_rotate_args(tfhe_context* ctx, const void* lwe_in, size_t batch, unsigned block, const void* tv, size_t tv_count,
                            const void* acc_in, size_t rotation_offset, const void* glwe_out, const void* lwe_extracted) {
  if (!lwe_in) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer");
  if ((tv != nullptr) == (acc_in != nullptr))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "pass either test_vector_poly or acc_in, not both and not neither");
  if (!glwe_out && !lwe_extracted) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "pass glwe_out, lwe_extracted or both");
  TFHE_TRY(check_batch(ctx, {lwe_in}, batch, tv_count, acc_in ? "acc_count" : "tv_count"));
  if (acc_in && rotation_offset >= 2 * (size_t)ctx->N)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "rotation_offset must be below 2N = " + std::to_string(2 * (size_t)ctx->N));
  if (!acc_in && rotation_offset != 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "rotation_offset goes with acc_in");
  TFHE_TRY(check_block(ctx, block));
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "no bootstrapping key loaded");
  return TFHE_OK;
}

int check_block_bootstrap_args(tfhe_context* ctx, const void* lwe_in, size_t batch, unsigned block, const void* tv, size_t tv_count,
                               const void* lwe_out) {
  TFHE_TRY(check_batch(ctx, {lwe_in, tv, lwe_out}, batch, tv_count, "tv_count"));
  TFHE_TRY(check_block(ctx, block));
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "no bootstrapping key loaded");
  return TFHE_OK;
}

hipError_t enqueue_block_rotate(tfhe_context* ctx, const u32* lwe_in, size_t batch, unsigned block, const u32* src, size_t count, bool glwe,
                                u32 offset, u32* glwe_out, u32* lwe_extracted) {
  // accumulators between the launches of a segmented rotation: the caller's output, or the workspace (sized by reserve)
  u32* state = glwe_out ? glwe_out : (batch <= ctx->ws_batch ? ctx->d_glwe_c.as<u32>() : nullptr);
  PbsParams P = ctx->pbs;
  P.acc_glwe = glwe ? 1u : 0u;
  P.acc_offset = offset;
  const size_t words = glwe ? glwe_words(ctx) : (size_t)ctx->N;
  return launch::block_rotate(ctx->stream, ctx->field, P, ctx->d_tw.as(), ctx->d_block_roots.as(), lwe_in, batch, src, count == 1 ? 0 : words,
                              ctx->d_bsk.as(), block, glwe_out, lwe_extracted, state, &ctx->side);
}

}  // namespace

int tfhe_block_rotate_max_block(tfhe_context* ctx, unsigned* max_block) {
  if (!ctx || !max_block) return TFHE_ERR_INVALID_ARGUMENT;
  return block_rotate_max_block(ctx, max_block);
}

int tfhe_block_blind_rotate_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned block,
                                         const uint32_t* test_vector_poly, size_t tv_count, const uint32_t* acc_in, size_t rotation_offset,
                                         uint32_t* glwe_out, uint32_t* lwe_extracted) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_block_rotate_args(ctx, lwe_in, batch, block, test_vector_poly, tv_count, acc_in, rotation_offset, glwe_out, lwe_extracted));
  TFHE_TRY(span_begin(ctx, kRotationSpan));
  HIP_TRY(ctx, enqueue_block_rotate(ctx, lwe_in, batch, block, acc_in ? acc_in : test_vector_poly, tv_count, acc_in != nullptr,
                                    (u32)rotation_offset, glwe_out, lwe_extracted));
  return span_end(ctx, kRotationSpan);
}

int tfhe_block_blind_rotate_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned block, const uint32_t* test_vector_poly,
                                  size_t tv_count, const uint32_t* acc_in, size_t rotation_offset, uint32_t* glwe_out,
                                  uint32_t* lwe_extracted) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_block_rotate_args(ctx, lwe_in, batch, block, test_vector_poly, tv_count, acc_in, rotation_offset, glwe_out, lwe_extracted));
  if (!acc_in) TFHE_TRY(check_tv_host(ctx, test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * lwe_words(ctx)));
  if (acc_in) TFHE_TRY(upload(ctx, ctx->d_glwe_a.as<u32>(), acc_in, tv_count * glwe_words(ctx)));
  else TFHE_TRY(upload(ctx, ctx->d_tv.as<u32>(), test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(tfhe_block_blind_rotate_batch_device(ctx, ctx->d_lwe_in.as<u32>(), batch, block, acc_in ? nullptr : ctx->d_tv.as<u32>(), tv_count,
                                                acc_in ? ctx->d_glwe_a.as<u32>() : nullptr, rotation_offset,
                                                glwe_out ? ctx->d_glwe_b.as<u32>() : nullptr, lwe_extracted ? ctx->d_lwe_big.as<u32>() : nullptr));
  if (glwe_out) TFHE_TRY(download(ctx, glwe_out, ctx->d_glwe_b.as<u32>(), batch * glwe_words(ctx)));
  if (lwe_extracted) TFHE_TRY(download(ctx, lwe_extracted, ctx->d_lwe_big.as<u32>(), batch * big_lwe_words(ctx)));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_OK;
}

int tfhe_block_bootstrap_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned block,
                                      const uint32_t* test_vector_poly, size_t tv_count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_block_bootstrap_args(ctx, lwe_in, batch, block, test_vector_poly, tv_count, lwe_out));
  TFHE_TRY(reserve(ctx, batch));  // (nothing to do after tfhe_context_reserve)
  return enqueue_bootstrap_with(ctx, lwe_in, batch, ctx->d_lwe_big.as<u32>(), lwe_out, [&](const u32* br_in, u32* br_out) {
    return enqueue_block_rotate(ctx, br_in, batch, block, test_vector_poly, tv_count, false, 0u, nullptr, br_out);
  });
}

int tfhe_block_bootstrap_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned block, const uint32_t* test_vector_poly,
                               size_t tv_count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_block_bootstrap_args(ctx, lwe_in, batch, block, test_vector_poly, tv_count, lwe_out));
  TFHE_TRY(check_tv_host(ctx, test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(reserve(ctx, batch));
  TFHE_TRY(upload(ctx, ctx->d_lwe_in.as<u32>(), lwe_in, batch * io_words(ctx)));
  TFHE_TRY(upload(ctx, ctx->d_tv.as<u32>(), test_vector_poly, tv_count * ctx->N));
  TFHE_TRY(tfhe_block_bootstrap_batch_device(ctx, ctx->d_lwe_in.as<u32>(), batch, block, ctx->d_tv.as<u32>(), tv_count, ctx->d_lwe_out.as<u32>()));
  return download_and_wait(ctx, lwe_out, ctx->d_lwe_out.as<u32>(), batch * io_words(ctx));
}

// ---------------------------------------------------------------------------------- multi-value bootstrap
// tfhe_hip.h states the operation, multi_value.h::sparse_extract_tile the per-table step.  ONE rotation of the constant
// accumulator per input, then one launch that turns the lookup tables into coefficient rows and one that combines the
// B + 1 sample extractions for every (input, table); in the reference's order the key switch runs over the combinations.
namespace {

struct MvLayout {
  size_t ks = 0, acc = 0, coeffs = 0, big = 0;  // offsets in words
  size_t words = 0;
};

void mv_layout(const tfhe_context* ctx, size_t batch, size_t tables, MvLayout* L) {
  auto pad = [](size_t w) { return (w + 3) & ~(size_t)3; };  // 16-byte buffers
  size_t at = 0;
  auto take = [&](size_t w) { const size_t o = at; at += pad(w); return o; };
  L->ks = take(batch * lwe_words(ctx));
  L->acc = take(batch * glwe_words(ctx));
  L->coeffs = take(batch * tables * (((size_t)1 << ctx->params.log_p) + 1));  // lut_sets = batch fits
  L->big = take(batch * tables * big_lwe_words(ctx));
  L->words = at;
}

size_t mv_bytes(const tfhe_context* ctx, size_t batch, size_t tables) {
  MvLayout L;
  mv_layout(ctx, batch, tables, &L);
  return L.words * sizeof(u32);
}

u32* mv_acc0(const tfhe_context* ctx) { return ctx->d_mv_const.as<u32>(); }
u32* mv_positions(const tfhe_context* ctx) { return ctx->d_mv_const.as<u32>() + glwe_words(ctx); }
u32* mv_caller_positions(const tfhe_context* ctx) { return ctx->d_mv_const.as<u32>() + glwe_words(ctx) + kSparseMaxTerms; }

// what the parameters must allow: kappa = 2^(31 - log_p - padding) exists, a value covers at least two coefficients
int check_mv_params(tfhe_context* ctx) {
  const tfhe_params& p = ctx->params;
  if (p.log_p + p.padding_bits > 31)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "multi-value bootstrapping needs log_p + padding_bits <= 31 (the accumulator holds half a step): " +
                    std::to_string(p.log_p + p.padding_bits));
  if (p.log_p >= ctx->pbs.log_n)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "multi-value bootstrapping needs log_p < log2 N (at least two coefficients per value)");
  return TFHE_OK;
}

int check_mv_shape(tfhe_context* ctx, size_t batch, size_t tables) {
  if (batch == 0 || tables == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch and tables must be at least 1");
  if (batch > kMaxBatch || tables > kMaxBatch || (double)batch * (double)tables > (double)kMaxBatch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch * tables exceeds 2^31 - 1 (one key switch per result)");
  return TFHE_OK;
}

// the constants of the context's multi-value calls; allocates once (never inside a _device form)
int ensure_mv_const(tfhe_context* ctx) {
  if (ctx->d_mv_const) return TFHE_OK;
  TFHE_TRY(check_mv_params(ctx));
  const tfhe_params& p = ctx->params;
  TFHE_TRY(ctx->d_mv_const.grow(ctx, (glwe_words(ctx) + 2 * (size_t)kSparseMaxTerms) * sizeof(u32)));
  hipError_t e = launch::multi_value_constants(ctx->stream, p.log_p, ctx->pbs.log_n, ctx->pbs.k, 1u << (31 - p.log_p - p.padding_bits),
                                               mv_acc0(ctx), mv_positions(ctx));
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the stream may be another one by the next call
  if (e != hipSuccess) {
    (void)ctx->d_mv_const.resize(ctx, 0);  // no constants: the next call starts over
    return hip_fail(ctx, e, "multi_value_constants");
  }
  return TFHE_OK;
}

int reserve_mv(tfhe_context* ctx, size_t batch, size_t tables) {
  TFHE_TRY(ensure_mv_const(ctx));
  if (batch <= ctx->mv_batch && tables <= ctx->mv_tables) return TFHE_OK;
  const size_t new_batch = std::max(batch, ctx->mv_batch), new_tables = std::max(tables, ctx->mv_tables);
  TFHE_TRY(check_mv_shape(ctx, new_batch, new_tables));
  ctx->mv_batch = ctx->mv_tables = 0;
  TFHE_TRY(ctx->d_mv_ws.grow(ctx, mv_bytes(ctx, new_batch, new_tables)));
  ctx->mv_batch = new_batch;
  ctx->mv_tables = new_tables;
  return TFHE_OK;
}

// steps 1 and 2 on rotation inputs [batch][n + 1]: A [batch][k+1][N] and coeffs [sets][tables][B + 1] are scratch,
// out [batch][tables][k N + 1].  The tree LUT's level 0 (tables = tables * B^(d-1) sub-tables) and the bootstrap share it;
// timed: the rotation goes between the rotation span's events, as in a bootstrap (the tree LUT times nothing).
int enqueue_mv_rotate_combine(tfhe_context* ctx, const u32* rot_in, size_t batch, const u32* luts, size_t lut_sets, size_t tables,
                              u32* A, u32* coeffs, u32* out, bool timed) {
  const u32 log_p = ctx->params.log_p;
  const size_t sets = lut_sets == 1 ? 1 : batch;
  if (timed) TFHE_TRY(span_begin(ctx, kRotationSpan));
  HIP_TRY(ctx, enqueue_blind_rotate(ctx, rot_in, batch, mv_acc0(ctx), 1, A, nullptr, AccSource{true, 0u}));
  if (timed) TFHE_TRY(span_end(ctx, kRotationSpan, false));
  HIP_TRY(ctx, launch::multi_value_coefficients(ctx->stream, luts, sets * tables, log_p, reinterpret_cast<i32*>(coeffs)));
  HIP_TRY(ctx, launch::glwe_sparse_extract(ctx->stream, A, batch, mv_positions(ctx), (1u << log_p) + 1u, reinterpret_cast<const i32*>(coeffs),
                                           sets != 1, (u32)tables, ctx->pbs.log_n, ctx->pbs.k, out));
  return TFHE_OK;
}

int check_mv_args(tfhe_context* ctx, const void* lwe_in, const void* luts, const void* lwe_out, size_t batch, size_t lut_sets, size_t tables) {
  TFHE_TRY(check_present(ctx, {lwe_in, luts, lwe_out}, 1, "null pointer"));
  TFHE_TRY(check_mv_shape(ctx, batch, tables));
  if (lut_sets != 1 && lut_sets != batch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "lut_sets must be 1 or batch");
  TFHE_TRY(check_mv_params(ctx));
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "load the bootstrapping key first");
  if (ctx->bmmp)
    return fail(ctx, TFHE_ERR_UNSUPPORTED,
                "a BMMP key is loaded: the shared rotation starts from a GLWE accumulator, which the unrolled rotation does not do");
  return TFHE_OK;
}

int check_sparse_args(tfhe_context* ctx, const void* glwe, size_t batch, const uint32_t* positions, size_t terms, const void* coeffs,
                      size_t sets, size_t tables, const void* lwe_out) {
  TFHE_TRY(check_present(ctx, {glwe, positions, coeffs, lwe_out}, 1, "null pointer"));
  TFHE_TRY(check_mv_shape(ctx, batch, tables));
  if (sets != 1 && sets != batch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "sets must be 1 or batch");
  if (terms == 0 || terms > ctx->N || terms > kSparseMaxTerms)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "terms must be in [1, N]: the positions are distinct and below N = " + std::to_string(ctx->N));
  std::vector<bool> seen(ctx->N, false);
  for (size_t m = 0; m < terms; ++m) {
    if (positions[m] >= ctx->N)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "position " + std::to_string(positions[m]) + " is not below N = " + std::to_string(ctx->N));
    if (seen[positions[m]]) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "position " + std::to_string(positions[m]) + " is repeated");
    seen[positions[m]] = true;
  }
  return TFHE_OK;
}

}  // namespace

int tfhe_context_reserve_multi_value(tfhe_context* ctx, size_t max_batch, size_t max_tables) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_mv_shape(ctx, max_batch, max_tables));
  return reserve_mv(ctx, max_batch, max_tables);
}

int tfhe_context_set_tree_lut_level0(tfhe_context* ctx, int multi_value) {
  TFHE_TRY(check_ctx(ctx));
  if (multi_value != 0 && multi_value != 1) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "multi_value must be 0 or 1");
  if (multi_value) TFHE_TRY(ensure_mv_const(ctx));
  ctx->tree_level0_multi_value = multi_value != 0;
  return TFHE_OK;
}

int tfhe_glwe_sparse_extract_batch_device(tfhe_context* ctx, const uint32_t* glwe, size_t batch, const uint32_t* positions, size_t terms,
                                          const int32_t* coeffs, size_t sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_sparse_args(ctx, glwe, batch, positions, terms, coeffs, sets, tables, lwe_out));
  if (!ctx->d_mv_const)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(terms * sizeof(u32)) +
                    " bytes for its positions on the device, 0 are reserved (tfhe_context_reserve_multi_value)");
  HIP_TRY(ctx, launch::sparse_positions(ctx->stream, positions, (u32)terms, mv_caller_positions(ctx)));
  HIP_TRY(ctx, launch::glwe_sparse_extract(ctx->stream, glwe, batch, mv_caller_positions(ctx), (u32)terms, coeffs, sets != 1,
                                           (u32)tables, ctx->pbs.log_n, ctx->pbs.k, lwe_out));
  return TFHE_OK;
}

int tfhe_glwe_sparse_extract_batch(tfhe_context* ctx, const uint32_t* glwe, size_t batch, const uint32_t* positions, size_t terms,
                                   const int32_t* coeffs, size_t sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_sparse_args(ctx, glwe, batch, positions, terms, coeffs, sets, tables, lwe_out));
  TFHE_TRY(ensure_mv_const(ctx));
  enum { kIn, kCoeffs, kOut };
  Staging s(ctx, {batch * glwe_words(ctx), sets * tables * terms, batch * tables * big_lwe_words(ctx)});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, glwe));
  TFHE_TRY(s.upload(kCoeffs, coeffs));
  TFHE_TRY(tfhe_glwe_sparse_extract_batch_device(ctx, s[kIn], batch, positions, terms, reinterpret_cast<const int32_t*>(s[kCoeffs]), sets,
                                                 tables, s[kOut]));
  return s.download_and_wait(kOut, lwe_out);
}

int tfhe_multi_value_bootstrap_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, const uint32_t* luts, size_t lut_sets,
                                            size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_mv_args(ctx, lwe_in, luts, lwe_out, batch, lut_sets, tables));
  if (!ctx->d_mv_const || batch > ctx->mv_batch || tables > ctx->mv_tables)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(mv_bytes(ctx, batch, tables)) + " bytes of multi-value workspace (batch " +
                    std::to_string(batch) + ", " + std::to_string(tables) + " tables), " +
                    std::to_string(ctx->mv_batch ? mv_bytes(ctx, ctx->mv_batch, ctx->mv_tables) : 0) + " are reserved for batch " +
                    std::to_string(ctx->mv_batch) + " and " + std::to_string(ctx->mv_tables) + " tables (tfhe_context_reserve_multi_value)");
  MvLayout L;
  mv_layout(ctx, ctx->mv_batch, ctx->mv_tables, &L);
  u32* ws = ctx->d_mv_ws.as<u32>();
  const u32 n = ctx->params.lwe_dimension;
  auto key_switch = [&](const u32* in, size_t count, u32* out) -> int {
    TFHE_TRY(span_begin(ctx, kKeySwitchSpan));
    HIP_TRY(ctx, launch::key_switch(ctx->stream, ctx->ks, ctx->big_n, n, in, count, ctx->d_ksk.as<u32>(), out, ctx->d_ksk_matrix.as(), ctx->ks_path));
    return span_end(ctx, kKeySwitchSpan, false);
  };
  if (ctx->ks_first) {
    TFHE_TRY(key_switch(lwe_in, batch, ws + L.ks));
    TFHE_TRY(enqueue_mv_rotate_combine(ctx, ws + L.ks, batch, luts, lut_sets, tables, ws + L.acc, ws + L.coeffs, lwe_out, true));
  } else {
    TFHE_TRY(enqueue_mv_rotate_combine(ctx, lwe_in, batch, luts, lut_sets, tables, ws + L.acc, ws + L.coeffs, ws + L.big, true));
    TFHE_TRY(key_switch(ws + L.big, batch * tables, lwe_out));  // after the combination: its noise is not amplified
  }
  if (ctx->timing) ctx->ev_valid_br = ctx->ev_valid_ks = true;  // both spans, as after a bootstrap
  return TFHE_OK;
}

int tfhe_multi_value_bootstrap_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, const uint32_t* luts, size_t lut_sets,
                                     size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_mv_args(ctx, lwe_in, luts, lwe_out, batch, lut_sets, tables));
  TFHE_TRY(reserve_mv(ctx, batch, tables));
  const size_t io = io_words(ctx);
  enum { kIn, kLuts, kOut };
  Staging s(ctx, {batch * io, lut_sets * tables << ctx->params.log_p, batch * tables * io});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, lwe_in));
  TFHE_TRY(s.upload(kLuts, luts));
  TFHE_TRY(tfhe_multi_value_bootstrap_batch_device(ctx, s[kIn], batch, s[kLuts], lut_sets, tables, s[kOut]));
  return s.download_and_wait(kOut, lwe_out);
}

// ---------------------------------------------------------------------------------- tree LUT
// tfhe_hip.h states the operation.  Level t is ONE rotation call over all rows x tables x sub-tables and one packing
// call (in the chunks the packing workspace holds, like tfhe_pack_lwe_batch_device); the only host loop is the one over
// the d levels.
//
// How the rotations of a level share a row's digit and -- at level 0 -- a (set, table)'s test vectors: EXPANDED BUFFERS
// in the reserved workspace, not an index map.  The rotate kernels address sample r's inputs at r * stride; an index map
// would be one more argument (and one more dependent load before the first CMUX) in every rotate kernel, team, pair and
// wide -- the kernels whose loops this feature promises to leave alone.  The copies are n + 1 + N words per rotation,
// about what a rotation writes back (k N + 1 words), written by two small kernels per call.
namespace {

constexpr size_t kTreeLutMaxBits = 16;  // d * log_p: the table has at most 2^16 entries per (set, table)

struct TreeLutLayout {
  size_t rotations = 0;  // level 0: batch * tables * B^(d-1)
  size_t ks_digit = 0, lwe = 0, tv = 0, state = 0, res_a = 0, res_b = 0, glwe = 0;  // offsets in words
  size_t words = 0;
};

// false: the sizes overflow / the first level does not fit one grid
bool tree_lut_layout(const tfhe_context* ctx, size_t batch, size_t digits, size_t tables, TreeLutLayout* L) {
  const u32 log_p = ctx->params.log_p;
  const double r0 = (double)batch * (double)tables * std::ldexp(1.0, (int)(log_p * (digits - 1)));
  if (r0 > (double)kMaxBatch) return false;
  const size_t R0 = batch * tables << (log_p * (digits - 1));
  const size_t G1 = digits > 1 ? R0 >> log_p : 0;
  const size_t n1 = lwe_words(ctx), big1 = big_lwe_words(ctx), glwe = glwe_words(ctx);
  auto pad = [](size_t w) { return (w + 3) & ~(size_t)3; };  // 16-byte buffers
  size_t at = 0;
  auto take = [&](size_t w) { const size_t o = at; at += pad(w); return o; };
  L->rotations = R0;
  L->ks_digit = take(batch * n1);  // reserved for either bootstrap order
  L->lwe = take(R0 * n1);
  L->tv = take(R0 * ctx->N);
  L->state = take(R0 * glwe);
  L->res_a = take(R0 * big1);
  L->res_b = take(G1 * big1);
  L->glwe = take(G1 * glwe);
  L->words = at;
  return true;
}

int check_tree_lut_shape(tfhe_context* ctx, size_t batch, size_t digits, size_t tables, TreeLutLayout* L) {
  const u32 log_p = ctx->params.log_p;
  if (batch == 0 || tables == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch and tables must be at least 1");
  if (log_p == 0 || log_p >= ctx->pbs.log_n)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the tree LUT needs 1 <= log_p < log2 N (at least two coefficients per value)");
  const size_t max_digits = kTreeLutMaxBits / log_p;
  if (digits == 0 || digits > max_digits)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "digits must be in [1, " + std::to_string(max_digits) + "]: d * log_p <= " + std::to_string(kTreeLutMaxBits));
  if (batch > kMaxBatch || tables > kMaxBatch || !tree_lut_layout(ctx, batch, digits, tables, L))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch * tables * B^(d-1) rotations exceed 2^31 - 1 (one workgroup per sample)");
  return TFHE_OK;
}

int check_tree_lut_keys(tfhe_context* ctx) {
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "load the bootstrapping key first");
  if (!ctx->have_pksk) return fail(ctx, TFHE_ERR_NO_KEY, "load a packing key first (tfhe_load_packing_key, from the flattened GLWE key)");
  if (ctx->pksk_dim != ctx->big_n)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the packing key packs from dimension " + std::to_string(ctx->pksk_dim) + ", the tree LUT packs sample extractions: k N = " +
                    std::to_string(ctx->big_n));
  if (ctx->bmmp)
    return fail(ctx, TFHE_ERR_UNSUPPORTED, "a BMMP key is loaded: the upper levels rotate a GLWE accumulator, which the unrolled rotation does not do");
  return TFHE_OK;
}

// everything a tree-LUT call is refused for before its workspace is looked at; -> the layout of the call
int check_tree_lut_args(tfhe_context* ctx, const uint32_t* const* digits, size_t d, size_t batch, const void* table,
                        size_t table_sets, size_t tables, const void* lwe_out, TreeLutLayout* L) {
  TFHE_TRY(check_present(ctx, {digits, table, lwe_out}, 1, "null pointer"));
  TFHE_TRY(check_tree_lut_shape(ctx, batch, d, tables, L));
  for (size_t t = 0; t < d; ++t)
    if (!digits[t]) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null digit pointer");
  if (table_sets != 1 && table_sets != batch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "table_sets must be 1 or batch");
  return check_tree_lut_keys(ctx);
}

}  // namespace

int tfhe_context_reserve_tree_lut(tfhe_context* ctx, size_t max_batch, size_t max_digits, size_t max_tables) {
  TFHE_TRY(check_ctx(ctx));
  TreeLutLayout L;
  TFHE_TRY(check_tree_lut_shape(ctx, max_batch, max_digits, max_tables, &L));
  return ctx->d_tree_ws.grow(ctx, L.words * sizeof(u32));
}

int tfhe_tree_lut_batch_device(tfhe_context* ctx, const uint32_t* const* digits, size_t d, size_t batch, const uint32_t* table,
                               size_t table_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TreeLutLayout L;
  TFHE_TRY(check_tree_lut_args(ctx, digits, d, batch, table, table_sets, tables, lwe_out, &L));
  if (L.words > ctx->d_tree_ws.words())
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(L.words * sizeof(u32)) + " bytes of tree-LUT workspace, " +
                    std::to_string(ctx->d_tree_ws.bytes()) + " are reserved (tfhe_context_reserve_tree_lut)");
  if (ctx->tree_level0_multi_value) TFHE_TRY(check_mv_params(ctx));
  const u32 log_p = ctx->params.log_p, log_n = ctx->pbs.log_n, n = ctx->params.lwe_dimension;
  const u32 log_rep = log_n - log_p;
  const size_t n1 = lwe_words(ctx);
  u32* ws = ctx->d_tree_ws.as<u32>();
  u32 *ks_digit = ws + L.ks_digit, *lwe = ws + L.lwe, *tv = ws + L.tv, *state = ws + L.state, *glwes = ws + L.glwe;
  u32* results[2] = {ws + L.res_a, ws + L.res_b};
  hipStream_t s = ctx->stream;
  // the digit a level rotates by, [batch][n+1]: key-switched first in the KS-first order
  auto digit_of = [&](size_t t, const u32** out) -> int {
    *out = digits[t];
    if (!ctx->ks_first) return TFHE_OK;
    HIP_TRY(ctx, launch::key_switch(s, ctx->ks, ctx->big_n, n, digits[t], batch, ctx->d_ksk.as<u32>(), ks_digit, ctx->d_ksk_matrix.as(), ctx->ks_path));
    *out = ks_digit;
    return TFHE_OK;
  };
  // level 0: rotation (row, table, h) bootstraps c_0[row] against sub-table h of (set, table)
  size_t count = L.rotations;
  const u32* digit = nullptr;
  TFHE_TRY(digit_of(0, &digit));
  u32* cur = d == 1 && ctx->ks_first ? lwe_out : results[0];
  if (ctx->tree_level0_multi_value) {
    // ONE rotation per row; the tables * B^(d-1) sub-tables of a row are coefficient rows of the per-table step, in the
    // order (table, h) of the table itself.  A sits where the segments' state would, the coefficients where the test
    // vectors would: (B + 1) words against N per sub-table.
    TFHE_TRY(enqueue_mv_rotate_combine(ctx, digit, batch, table, table_sets, count / batch, state, tv, cur, false));
  } else {
    HIP_TRY(ctx, launch::tree_lut_expand(s, digit, count, count / batch, (u32)n1, lwe));
    HIP_TRY(ctx, launch::tree_lut_test_vectors(s, table, table_sets == 1 ? 0 : tables << (log_p * d), count, count / batch, log_p, log_n, tv));
    HIP_TRY(ctx, enqueue_blind_rotate(ctx, lwe, count, tv, count, nullptr, cur, AccSource{false, 0u, state}));
  }
  for (size_t t = 1; t < d; ++t) {
    // G_h = Pack of the B results [h B, (h + 1) B), each on N / B neighbouring coefficients
    const size_t groups = count >> log_p;
    TFHE_TRY(enqueue_pack(ctx, cur, groups, 1u << log_p, glwes, log_rep));
    TFHE_TRY(digit_of(t, &digit));
    HIP_TRY(ctx, launch::tree_lut_expand(s, digit, groups, groups / batch, (u32)n1, lwe));
    u32* next = t + 1 == d && ctx->ks_first ? lwe_out : results[t & 1];
    HIP_TRY(ctx, enqueue_blind_rotate(ctx, lwe, groups, glwes, groups, nullptr, next, AccSource{true, (1u << log_rep) >> 1, state}));
    cur = next;
    count = groups;
  }
  if (!ctx->ks_first) HIP_TRY(ctx, launch::key_switch(s, ctx->ks, ctx->big_n, n, cur, count, ctx->d_ksk.as<u32>(), lwe_out, ctx->d_ksk_matrix.as(), ctx->ks_path));
  return TFHE_OK;
}

int tfhe_tree_lut_batch(tfhe_context* ctx, const uint32_t* const* digits, size_t d, size_t batch, const uint32_t* table,
                        size_t table_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TreeLutLayout L;
  TFHE_TRY(check_tree_lut_args(ctx, digits, d, batch, table, table_sets, tables, lwe_out, &L));
  TFHE_TRY(tfhe_context_reserve_tree_lut(ctx, batch, d, tables));
  const size_t io = io_words(ctx);
  std::vector<size_t> words(d, batch * io);  // segments 0 .. d-1: the digits; then the table and the result
  words.push_back(table_sets * tables << (ctx->params.log_p * d));
  words.push_back(batch * tables * io);
  Staging s(ctx, words);
  TFHE_TRY(s.reserve());
  std::vector<const uint32_t*> ptrs(d);
  for (size_t t = 0; t < d; ++t) {
    TFHE_TRY(s.upload(t, digits[t]));
    ptrs[t] = s[t];
  }
  TFHE_TRY(s.upload(d, table));
  TFHE_TRY(tfhe_tree_lut_batch_device(ctx, ptrs.data(), d, batch, s[d], table_sets, tables, s[d + 1]));
  return s.download_and_wait(d + 1, lwe_out);
}

// ---------------------------------------------------------------------------------- digit extraction, wide LUT
// tfhe_hip.h states the operation, lwe_extract.h::extract_step the launch between two bootstraps.  The only host loop
// is the one over the w bits: one bootstrap call and one step launch each.
namespace {

constexpr unsigned kExtractMaxBits = 16;

struct ExtractShape {
  size_t batch;
  unsigned lsb, g, d, out_lsb;
};

struct ExtractLayout {
  size_t r = 0, s = 0, o = 0, acc = 0, digits = 0, digit_stride = 0;  // offsets in words
  size_t words = 0;
};

// every row at the larger boundary dimension, so that switching the bootstrap order keeps a reservation valid
void extract_layout(const tfhe_context* ctx, size_t batch, size_t digits, ExtractLayout* out) {
  auto pad = [](size_t w) { return (w + 3) & ~(size_t)3; };  // 16-byte buffers
  ExtractLayout& L = *out;
  L.digit_stride = pad(batch * std::max(lwe_words(ctx), big_lwe_words(ctx)));
  L.r = 0;
  L.s = L.digit_stride;
  L.o = 2 * L.digit_stride;
  L.acc = 3 * L.digit_stride;
  L.digits = L.acc + pad(glwe_words(ctx));
  L.words = L.digits + digits * L.digit_stride;
}

size_t extract_bytes(const tfhe_context* ctx, size_t batch, size_t digits) {
  ExtractLayout L;
  extract_layout(ctx, batch, digits, &L);
  return L.words * sizeof(u32);
}

int check_extract_shape(tfhe_context* ctx, const ExtractShape& e) {
  if (e.batch == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "empty batch");
  if (e.batch > kMaxBatch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "batch exceeds 2^31 - 1 (one workgroup per sample)");
  if (e.g == 0 || e.d == 0 || e.g > kExtractMaxBits || e.d > kExtractMaxBits || e.g * e.d > kExtractMaxBits)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "digit_bits and digits must be at least 1 and w = digit_bits * digits at most " + std::to_string(kExtractMaxBits));
  if (e.lsb == 0 || e.out_lsb == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "lsb and out_lsb must be at least 1 (bit m - 1 holds the constant)");
  if (e.lsb > 32 || e.lsb + e.g * e.d > 32)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "lsb + w <= 32 is required: lsb = " + std::to_string(e.lsb) + ", w = " + std::to_string(e.g * e.d));
  if (e.out_lsb > 32 || e.out_lsb + e.g > 32)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "out_lsb + digit_bits <= 32 is required: out_lsb = " + std::to_string(e.out_lsb) + ", digit_bits = " + std::to_string(e.g));
  return TFHE_OK;
}

int reserve_extract(tfhe_context* ctx, size_t batch, size_t digits) {
  TFHE_TRY(reserve(ctx, batch));
  if (batch <= ctx->extract_batch && digits <= ctx->extract_digits) return TFHE_OK;
  const size_t new_batch = std::max(batch, ctx->extract_batch), new_digits = std::max(digits, ctx->extract_digits);
  ctx->extract_batch = ctx->extract_digits = 0;
  TFHE_TRY(ctx->d_extract_ws.grow(ctx, extract_bytes(ctx, new_batch, new_digits)));
  ctx->extract_batch = new_batch;
  ctx->extract_digits = new_digits;
  return TFHE_OK;
}

// the call fits what is reserved, with `ws_digits` digit buffers of the workspace in use (0: the caller's own)
int check_extract_reserved(tfhe_context* ctx, size_t batch, size_t ws_digits) {
  if (batch <= ctx->extract_batch && ws_digits <= ctx->extract_digits && batch <= ctx->ws_batch) return TFHE_OK;
  return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
              "the call needs " + std::to_string(extract_bytes(ctx, batch, ws_digits)) +
                  " bytes of extraction workspace (batch " + std::to_string(batch) + ", " + std::to_string(ws_digits) +
                  " digit buffers), " +
                  std::to_string(ctx->extract_batch && batch <= ctx->ws_batch ? ctx->d_extract_ws.bytes() : 0) +
                  " are reserved (tfhe_context_reserve_extract)");
}

// the w sign bootstraps and the w + 1 step launches; everything has been checked
int enqueue_extract(tfhe_context* ctx, const u32* lwe_in, const ExtractShape& e, u32* const* digits_out, u32* remainder_out) {
  ExtractLayout L;
  extract_layout(ctx, ctx->extract_batch, ctx->extract_digits, &L);
  u32 *r = ctx->d_extract_ws.as<u32>() + L.r, *s = ctx->d_extract_ws.as<u32>() + L.s, *o = ctx->d_extract_ws.as<u32>() + L.o, *acc = ctx->d_extract_ws.as<u32>() + L.acc;
  const u32 w = e.g * e.d;
  auto m_of = [&](u32 j) { return std::min(e.lsb + j, e.out_lsb + j % e.g); };
  ExtractStepArgs a{};
  a.total = e.batch * io_words(ctx);
  a.words = (u32)io_words(ctx);
  a.acc_words = (u32)glwe_words(ctx);
  a.acc_body = ctx->big_n;
  // r_0 = lwe_in, s_0, the constant of bit 0
  a.r_in = lwe_in;
  a.r_out = r;
  a.s_out = s;
  a.acc = acc;
  a.s_shift = 31u - e.lsb;
  a.acc_kappa = 1u << (m_of(0) - 1);
  HIP_TRY(ctx, launch::extract_step(ctx->stream, a));
  for (u32 j = 0; j < w; ++j) {
    TFHE_TRY(enqueue_bootstrap(ctx, s, e.batch, acc, 1, ctx->d_lwe_big.as<u32>(), o, AccSource{true, ctx->N / 2}));
    const u32 i = j % e.g, m = m_of(j);
    const bool last = j + 1 == w;
    a.r_in = r;
    a.o = o;
    a.r_out = last ? remainder_out : r;
    a.s_out = last ? nullptr : s;
    a.digit = digits_out[j / e.g];
    a.acc = last ? nullptr : acc;
    a.kappa = 1u << (m - 1);
    a.r_shift = e.lsb + j - m;
    a.d_shift = e.out_lsb + i - m;
    a.s_shift = last ? 0u : 31u - e.lsb - (j + 1);
    a.d_keep = i ? 0xFFFFFFFFu : 0u;
    a.acc_kappa = last ? 0u : 1u << (m_of(j + 1) - 1);
    HIP_TRY(ctx, launch::extract_step(ctx->stream, a));
  }
  return TFHE_OK;
}

// everything an extraction is refused for before its workspace is looked at
int check_extract_args(tfhe_context* ctx, const void* lwe_in, const ExtractShape& e, uint32_t* const* digits_out, const void* remainder_out,
                       bool device) {
  TFHE_TRY(check_present(ctx, {lwe_in, digits_out}, 1, "null pointer"));
  TFHE_TRY(check_extract_shape(ctx, e));
  const size_t words = e.batch * io_words(ctx);
  for (unsigned t = 0; t < e.d; ++t) {
    if (!digits_out[t]) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null digit pointer");
    for (unsigned u = 0; u < t; ++u)
      if (overlap(digits_out[t], words, digits_out[u], words)) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "two digit buffers overlap");
    if (remainder_out && overlap(digits_out[t], words, remainder_out, words))
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "a digit buffer overlaps remainder_out");
    if (device && overlap(digits_out[t], words, lwe_in, words))
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "a digit buffer overlaps lwe_in");
  }
  // the bootstraps' own refusals: a key, and a plain one (the rotations start from a GLWE accumulator)
  const size_t offset = ctx->N / 2;
  return check_rotate_args(ctx, lwe_in, lwe_in, lwe_in, e.batch, 1, &offset);
}

// the wide LUT's fixed arguments of the extraction
ExtractShape wide_lut_shape(const tfhe_context* ctx, size_t batch, unsigned lsb, size_t d) {
  const u32 log_p = ctx->params.log_p, used = log_p + ctx->params.padding_bits;
  return ExtractShape{batch, lsb, log_p, (unsigned)std::min<size_t>(d, kExtractMaxBits + 1), used < 32 ? 32 - used : 0};
}

int check_wide_lut_args(tfhe_context* ctx, const void* lwe_in, size_t batch, unsigned lsb, size_t d, const void* table,
                        size_t table_sets, size_t tables, const void* lwe_out, TreeLutLayout* L) {
  TFHE_TRY(check_present(ctx, {lwe_in, table, lwe_out}, 1, "null pointer"));
  TFHE_TRY(check_tree_lut_shape(ctx, batch, d, tables, L));
  TFHE_TRY(check_extract_shape(ctx, wide_lut_shape(ctx, batch, lsb, d)));
  if (table_sets != 1 && table_sets != batch) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "table_sets must be 1 or batch");
  return check_tree_lut_keys(ctx);
}

}  // namespace

int tfhe_context_reserve_extract(tfhe_context* ctx, size_t max_batch, size_t max_digits) {
  TFHE_TRY(check_ctx(ctx));
  if (max_batch == 0 || max_batch > kMaxBatch || max_digits == 0 || max_digits > kExtractMaxBits)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "max_batch must be in [1, 2^31 - 1] and max_digits in [1, " + std::to_string(kExtractMaxBits) + "]");
  return reserve_extract(ctx, max_batch, max_digits);
}

int tfhe_context_reserve_wide_lut(tfhe_context* ctx, size_t max_batch, size_t max_digits, size_t max_tables) {
  TFHE_TRY(check_ctx(ctx));
  TreeLutLayout L;
  TFHE_TRY(check_tree_lut_shape(ctx, max_batch, max_digits, max_tables, &L));
  TFHE_TRY(reserve_extract(ctx, max_batch, max_digits));
  return tfhe_context_reserve_tree_lut(ctx, max_batch, max_digits, max_tables);
}

int tfhe_extract_digits_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned lsb, unsigned digit_bits,
                                     unsigned digits, unsigned out_lsb, uint32_t* const* digits_out, uint32_t* remainder_out) {
  TFHE_TRY(check_ctx(ctx));
  const ExtractShape e{batch, lsb, digit_bits, digits, out_lsb};
  TFHE_TRY(check_extract_args(ctx, lwe_in, e, digits_out, remainder_out, true));
  TFHE_TRY(check_extract_reserved(ctx, batch, 0));
  return enqueue_extract(ctx, lwe_in, e, digits_out, remainder_out);
}

int tfhe_extract_digits_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned lsb, unsigned digit_bits,
                              unsigned digits, unsigned out_lsb, uint32_t* const* digits_out, uint32_t* remainder_out) {
  TFHE_TRY(check_ctx(ctx));
  const ExtractShape e{batch, lsb, digit_bits, digits, out_lsb};
  TFHE_TRY(check_extract_args(ctx, lwe_in, e, digits_out, remainder_out, false));
  TFHE_TRY(reserve_extract(ctx, batch, digits));
  const size_t words = batch * io_words(ctx);
  // rows have an odd number of words: a gap keeps the remainder at the input's offset from a 16-byte boundary, so that
  // the last step launch moves 16 bytes per access like the others
  enum { kIn, kGap, kRemainder };
  Staging s(ctx, {words, (4 - words % 4) % 4, remainder_out ? words : 0});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, lwe_in));
  ExtractLayout L;
  extract_layout(ctx, ctx->extract_batch, ctx->extract_digits, &L);
  std::vector<u32*> ptrs(digits);
  for (unsigned t = 0; t < digits; ++t) ptrs[t] = ctx->d_extract_ws.as<u32>() + L.digits + t * L.digit_stride;
  TFHE_TRY(enqueue_extract(ctx, s[kIn], e, ptrs.data(), remainder_out ? s[kRemainder] : nullptr));
  for (unsigned t = 0; t < digits; ++t) TFHE_TRY(download(ctx, digits_out[t], ptrs[t], words));
  if (remainder_out) TFHE_TRY(download(ctx, remainder_out, s[kRemainder], words));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_OK;
}

int tfhe_wide_lut_batch_device(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned lsb, size_t d, const uint32_t* table,
                               size_t table_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TreeLutLayout TL;
  TFHE_TRY(check_wide_lut_args(ctx, lwe_in, batch, lsb, d, table, table_sets, tables, lwe_out, &TL));
  TFHE_TRY(check_extract_reserved(ctx, batch, d));
  if (TL.words > ctx->d_tree_ws.words())
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "the call needs " + std::to_string(TL.words * sizeof(u32)) + " bytes of tree-LUT workspace, " +
                    std::to_string(ctx->d_tree_ws.bytes()) + " are reserved (tfhe_context_reserve_wide_lut)");
  ExtractLayout L;
  extract_layout(ctx, ctx->extract_batch, ctx->extract_digits, &L);
  std::vector<u32*> ptrs(d);
  for (size_t t = 0; t < d; ++t) ptrs[t] = ctx->d_extract_ws.as<u32>() + L.digits + t * L.digit_stride;
  TFHE_TRY(enqueue_extract(ctx, lwe_in, wide_lut_shape(ctx, batch, lsb, d), ptrs.data(), nullptr));
  return tfhe_tree_lut_batch_device(ctx, ptrs.data(), d, batch, table, table_sets, tables, lwe_out);
}

int tfhe_wide_lut_batch(tfhe_context* ctx, const uint32_t* lwe_in, size_t batch, unsigned lsb, size_t d, const uint32_t* table,
                        size_t table_sets, size_t tables, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TreeLutLayout TL;
  TFHE_TRY(check_wide_lut_args(ctx, lwe_in, batch, lsb, d, table, table_sets, tables, lwe_out, &TL));
  TFHE_TRY(tfhe_context_reserve_wide_lut(ctx, batch, d, tables));
  const size_t io = io_words(ctx);
  enum { kIn, kTable, kOut };
  Staging s(ctx, {batch * io, table_sets * tables << (ctx->params.log_p * d), batch * tables * io});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, lwe_in));
  TFHE_TRY(s.upload(kTable, table));
  TFHE_TRY(tfhe_wide_lut_batch_device(ctx, s[kIn], batch, lsb, d, s[kTable], table_sets, tables, s[kOut]));
  return s.download_and_wait(kOut, lwe_out);
}

// ---------------------------------------------------------------------------------- radix integers
// tfhe_hip.h states the operations, radix.h::radix_glue the launch in front of every bootstrap level.  A level is one
// glue launch and one bootstrap call with an accumulator per rotation; the host loops below are over the levels only.
namespace {

struct RadixShape {
  u32 m, log_rep, log_delta;
};

// log_p = 2 m >= 4, a padding bit, and every block value on rep >= 2 coefficients
int check_radix_params(tfhe_context* ctx, RadixShape* shape) {
  const tfhe_params& p = ctx->params;
  if (p.log_p < 4 || p.log_p % 2 != 0)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "radix integers need log_p = 2 m with m >= 2, got log_p = " + std::to_string(p.log_p));
  if (p.padding_bits == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "radix integers need padding_bits >= 1");
  if (p.log_p + p.padding_bits > p.glwe_poly_degree)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                "radix integers need rep = N / 2^(log_p + padding_bits - 1) >= 2 coefficients per block value (P <= N / 2)");
  shape->m = p.log_p / 2;
  shape->log_rep = p.glwe_poly_degree + 1 - p.log_p - p.padding_bits;
  shape->log_delta = 32 - p.log_p - p.padding_bits;
  return TFHE_OK;
}

int check_radix_size(tfhe_context* ctx, size_t batch, size_t blocks) {
  if (batch == 0) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "empty batch");
  if (blocks == 0 || blocks > kRadixMaxBlocks)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "blocks must be in [1, " + std::to_string(kRadixMaxBlocks) + "]");
  if (batch > kMaxBatch / (2 * blocks))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "2 * batch * blocks exceeds 2^31 - 1 (one workgroup per rotation)");
  return TFHE_OK;
}

struct RadixLayout {
  size_t x = 0, o = 0, w = 0, s = 0, acc = 0;  // offsets in words
  size_t words = 0;
};

// every row at the larger boundary dimension, so that switching the bootstrap order keeps a reservation valid
void radix_layout(const tfhe_context* ctx, size_t batch, size_t blocks, RadixLayout* out) {
  auto pad = [](size_t w) { return (w + 3) & ~(size_t)3; };  // 16-byte buffers
  const size_t row = std::max(lwe_words(ctx), big_lwe_words(ctx)), half = pad(batch * blocks * row);
  RadixLayout& L = *out;
  L.x = 0;
  L.o = 2 * half;
  L.w = 4 * half;
  L.s = 5 * half;
  L.acc = 6 * half;
  L.words = L.acc + 2 * batch * blocks * glwe_words(ctx);
}

size_t radix_bytes(const tfhe_context* ctx, size_t batch, size_t blocks) {
  RadixLayout L;
  radix_layout(ctx, batch, blocks, &L);
  return L.words * sizeof(u32);
}

int reserve_radix(tfhe_context* ctx, size_t batch, size_t blocks) {
  RadixShape shape;
  TFHE_TRY(check_radix_params(ctx, &shape));
  if (!ctx->d_radix_tables) {  // once: the tables depend on the parameters only
    const u32 P = 1u << ctx->params.log_p;
    std::vector<u32> tables((size_t)kRadixTables * P);
    for (u32 t = 0; t < kRadixTables; ++t)
      for (u32 x = 0; x < P; ++x) tables[(size_t)t * P + x] = radix_table_value(t, shape.m, x);
    TFHE_TRY(ctx->d_radix_tables.grow(ctx, tables.size() * sizeof(u32)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_radix_tables.as(), tables.data(), tables.size() * sizeof(u32), hipMemcpyHostToDevice));
  }
  const size_t new_batch = std::max(batch, ctx->radix_batch), new_blocks = std::max(blocks, ctx->radix_blocks);
  TFHE_TRY(reserve(ctx, 2 * new_batch * new_blocks));
  if (batch <= ctx->radix_batch && blocks <= ctx->radix_blocks) return TFHE_OK;
  ctx->radix_batch = ctx->radix_blocks = 0;
  TFHE_TRY(ctx->d_radix_ws.grow(ctx, radix_bytes(ctx, new_batch, new_blocks)));
  ctx->radix_batch = new_batch;
  ctx->radix_blocks = new_blocks;
  return TFHE_OK;
}

int check_radix_reserved(tfhe_context* ctx, size_t batch, size_t blocks) {
  const bool base = 2 * ctx->radix_batch * ctx->radix_blocks <= ctx->ws_batch && ctx->d_radix_tables;
  if (base && batch <= ctx->radix_batch && blocks <= ctx->radix_blocks) return TFHE_OK;
  return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
              "the call needs " + std::to_string(radix_bytes(ctx, batch, blocks)) + " bytes of radix workspace (batch " +
                  std::to_string(batch) + ", " + std::to_string(blocks) + " blocks), " +
                  std::to_string(base && ctx->radix_batch ? ctx->d_radix_ws.bytes() : 0) + " are reserved (tfhe_context_reserve_radix)");
}

// the keys every level needs: a plain bootstrapping key (the rotations start from GLWE accumulators)
int check_radix_keys(tfhe_context* ctx) {
  const size_t offset = 0;
  return check_rotate_args(ctx, ctx, ctx, ctx, 1, 1, &offset);
}

// `out` [words] is `in` exactly, or apart from it
int check_radix_in_place(tfhe_context* ctx, const void* out, const void* in, size_t in_words, size_t out_words, const char* name) {
  if (!in || out == in || !overlap(out, out_words, in, in_words)) return TFHE_OK;
  return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, std::string("the output overlaps ") + name + " without being exactly in place");
}

// One level: the glue launch, then the bootstrap of its `rotations` outputs x with their accumulators into `out`.
struct RadixLevels {
  tfhe_context* ctx;
  RadixShape shape;
  size_t rows;
  u32 *x, *o, *w, *s, *acc;

  RadixLevels(tfhe_context* c, const RadixShape& sh, size_t r) : ctx(c), shape(sh), rows(r) {
    RadixLayout L;
    radix_layout(ctx, ctx->radix_batch, ctx->radix_blocks, &L);
    u32* ws = ctx->d_radix_ws.as<u32>();
    x = ws + L.x, o = ws + L.o, w = ws + L.w, s = ws + L.s, acc = ws + L.acc;
  }
  // a caller's integer [row][block] of `blocks` blocks, or a workspace buffer [block][row]
  RadixOperand rows_of(const u32* p, size_t blocks, u32 weight) const {
    return RadixOperand{p, (u32)blocks, 1u, -1, 1, 0, (u32)blocks, weight};
  }
  RadixOperand columns_of(const u32* p, size_t blocks, u32 weight, i32 mul = 1, i32 shift = 0) const {
    return RadixOperand{p, 1u, (u32)rows, -1, mul, shift, (u32)blocks, weight};
  }
  RadixGlueArgs glue(const RadixOperand& a, const RadixOperand& b, u32 j0, u32 nj, bool out_rows, u32* out) const {
    RadixGlueArgs g{};
    g.a = a;
    g.b = b;
    g.out = out;
    g.acc = acc;
    g.tables = ctx->d_radix_tables.as<u32>();
    g.rows = (u32)rows, g.j0 = j0, g.nj = nj, g.nt = 1;
    g.out_stride_q = out_rows ? nj : 1u;
    g.out_stride_j = out_rows ? 1u : (u32)rows;
    g.out_stride_t = nj * (u32)rows;
    g.words = (u32)io_words(ctx);
    g.acc_words = (u32)glwe_words(ctx);
    g.acc_body = ctx->big_n;
    g.log_rep = shape.log_rep, g.log_delta = shape.log_delta;
    g.table_words = 1u << ctx->params.log_p;
    return g;
  }
  void tables(RadixGlueArgs* g, u32 first, u32 count, u32 table) const {
    for (u32 j = first; j < first + count; ++j) g->sel[j] = (unsigned char)table;
  }
  int run(const RadixGlueArgs& g, const u32* in, size_t rotations, u32* out) const {
    HIP_TRY(ctx, launch::radix_glue(ctx->stream, g));
    return enqueue_bootstrap(ctx, in, rotations, acc, rotations, ctx->d_lwe_big.as<u32>(), out, AccSource{true, (1u << shape.log_rep) / 2});
  }
};

int enqueue_radix_propagate(tfhe_context* ctx, const RadixShape& shape, const u32* in, size_t rows, u32 D, u32* out) {
  const RadixLevels L(ctx, shape, rows);
  const RadixOperand none{};
  const size_t ct = rows * io_words(ctx);  // words of one block of every row
  // level 1: the message and (D > 1) the carry of every block
  RadixGlueArgs g = L.glue(L.rows_of(in, D, 1), none, 0, D, D == 1, L.x);
  g.nt = D == 1 ? 1 : 2;
  L.tables(&g, 0, D, kRadixMessage);
  TFHE_TRY(L.run(g, L.x, g.nt * D * rows, D == 1 ? out : L.o));
  if (D == 1) return TFHE_OK;
  // w_j = M_j + C_(j-1); level 2: the states of blocks 0 .. D-2
  g = L.glue(L.columns_of(L.o, D, 1), L.columns_of(L.o + D * ct, D, 1, 1, 1), 0, D, false, L.w);
  L.tables(&g, 0, 1, kRadixFirstState);
  L.tables(&g, 1, D - 2, kRadixState);
  L.tables(&g, D - 1, 1, kRadixNoTable);
  TFHE_TRY(L.run(g, L.w, (D - 1) * rows, L.s));
  // prefix levels: blocks below r are complete and stay where they are
  for (u32 r = 1; r < D - 1; r *= 2) {
    const u32 nj = D - 1 - r;
    g = L.glue(L.columns_of(L.s, D - 1, 4), L.columns_of(L.s, D - 1, 1, 1, (i32)r), r, nj, false, L.x);
    L.tables(&g, 0, std::min(r, nj), kRadixPrefixCarry);
    if (nj > r) L.tables(&g, r, nj - r, kRadixPrefixState);
    TFHE_TRY(L.run(g, L.x, nj * rows, L.s + r * ct));
  }
  // the carries enter: out_j = (w_j + S_(j-1)) mod Bm
  g = L.glue(L.columns_of(L.w, D, 1), L.columns_of(L.s, D - 1, 1, 1, 1), 0, D, true, L.x);
  L.tables(&g, 0, D, kRadixMessage);
  return L.run(g, L.x, D * rows, out);
}

int enqueue_radix_compare(tfhe_context* ctx, const RadixShape& shape, const u32* a, const u32* b, size_t rows, u32 D, u32 predicate, u32* out) {
  const RadixLevels L(ctx, shape, rows);
  const size_t ct = rows * io_words(ctx);
  RadixGlueArgs g = L.glue(L.rows_of(a, D, 1u << shape.m), L.rows_of(b, D, 1), 0, D, D == 1, L.x);
  L.tables(&g, 0, D, D == 1 ? kRadixComparePred + predicate : kRadixCompare);
  TFHE_TRY(L.run(g, L.x, D * rows, D == 1 ? out : L.s));
  for (u32 c = D; c > 1; c = c / 2 + c % 2) {
    // pairs (2j + 1, 2j) into j; with an odd count block 0 passes through and pairs (2j, 2j - 1) go into j >= 1
    const u32 odd = c % 2, pairs = c / 2;
    const bool last = pairs + odd == 1;
    g = L.glue(L.columns_of(L.s, c, 4, 2, odd ? 0 : -1), L.columns_of(L.s, c, 1, 2, odd ? 1 : 0), odd, pairs, false, L.x);
    L.tables(&g, 0, pairs, last ? kRadixTreePred + predicate : kRadixTree);
    TFHE_TRY(L.run(g, L.x, pairs * rows, last ? out : L.s + odd * ct));
  }
  return TFHE_OK;
}

struct RadixMapArgs {
  const u32 *a, *b;
  size_t a_blocks, b_blocks;
  u32 wa, wb;
  i32 a_shift, a_fixed, b_shift, b_fixed;
  size_t batch, blocks;
  const u32* tables;
  size_t table_count;
  const u32* sel;
  u32* out;
};

int check_radix_map(tfhe_context* ctx, const RadixMapArgs& m, RadixShape* shape) {
  TFHE_TRY(check_present(ctx, {m.a, m.tables, m.sel, m.out}, 1, "null pointer"));
  TFHE_TRY(check_radix_params(ctx, shape));
  TFHE_TRY(check_radix_size(ctx, m.batch, m.blocks));
  if (m.a_blocks == 0 || m.a_blocks > kRadixMaxBlocks || (m.b && (m.b_blocks == 0 || m.b_blocks > kRadixMaxBlocks)))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "a_blocks and b_blocks must be in [1, " + std::to_string(kRadixMaxBlocks) + "]");
  if (m.a_fixed >= (i64)m.a_blocks || (m.b && m.b_fixed >= (i64)m.b_blocks))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "a broadcast block index is out of range");
  if (m.table_count == 0 || m.table_count > kRadixNoTable)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "table_count must be in [1, " + std::to_string(kRadixNoTable) + "]");
  for (size_t j = 0; j < m.blocks; ++j)
    if (m.sel[j] >= m.table_count) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "table index " + std::to_string(m.sel[j]) + " of block " + std::to_string(j) + " is out of range");
  const size_t io = io_words(ctx), out_words = m.batch * m.blocks * io;
  TFHE_TRY(check_radix_in_place(ctx, m.out, m.a, m.batch * m.a_blocks * io, out_words, "a"));
  TFHE_TRY(check_radix_in_place(ctx, m.out, m.b, m.batch * m.b_blocks * io, out_words, "b"));
  return check_radix_keys(ctx);
}

int enqueue_radix_map(tfhe_context* ctx, const RadixShape& shape, const RadixMapArgs& m) {
  const RadixLevels L(ctx, shape, m.batch);
  RadixOperand a = L.rows_of(m.a, m.a_blocks, m.wa), b = L.rows_of(m.b, m.b ? m.b_blocks : 0, m.wb);
  a.fixed = m.a_fixed < 0 ? -1 : m.a_fixed, a.shift = m.a_shift;
  b.fixed = m.b_fixed < 0 ? -1 : m.b_fixed, b.shift = m.b_shift;
  RadixGlueArgs g = L.glue(a, b, 0, (u32)m.blocks, true, L.x);
  g.tables = m.tables;
  for (size_t j = 0; j < m.blocks; ++j) g.sel[j] = (unsigned char)m.sel[j];
  return L.run(g, L.x, m.blocks * m.batch, m.out);
}

int check_radix_propagate(tfhe_context* ctx, const void* in, size_t batch, size_t blocks, const void* out, RadixShape* shape) {
  TFHE_TRY(check_present(ctx, {in, out}, 1, "null pointer"));
  TFHE_TRY(check_radix_params(ctx, shape));
  TFHE_TRY(check_radix_size(ctx, batch, blocks));
  const size_t words = batch * blocks * io_words(ctx);
  TFHE_TRY(check_radix_in_place(ctx, out, in, words, words, "blocks_in"));
  return check_radix_keys(ctx);
}

int check_radix_compare(tfhe_context* ctx, const void* a, const void* b, size_t batch, size_t blocks, unsigned predicate, const void* out,
                        RadixShape* shape) {
  TFHE_TRY(check_present(ctx, {a, b, out}, 1, "null pointer"));
  TFHE_TRY(check_radix_params(ctx, shape));
  TFHE_TRY(check_radix_size(ctx, batch, blocks));
  if (predicate > TFHE_RADIX_GE) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "predicate must be one of TFHE_RADIX_EQ .. TFHE_RADIX_GE");
  const size_t io = io_words(ctx);
  // the result is written by the last level only, after every read of a and b: row 0 of either is "in place"
  TFHE_TRY(check_radix_in_place(ctx, out, a, batch * blocks * io, batch * io, "a"));
  TFHE_TRY(check_radix_in_place(ctx, out, b, batch * blocks * io, batch * io, "b"));
  return check_radix_keys(ctx);
}

}  // namespace

int tfhe_context_reserve_radix(tfhe_context* ctx, size_t max_batch, size_t max_blocks) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_radix_size(ctx, max_batch, max_blocks));
  return reserve_radix(ctx, max_batch, max_blocks);
}

int tfhe_radix_propagate_batch_device(tfhe_context* ctx, const uint32_t* blocks_in, size_t batch, size_t blocks, uint32_t* blocks_out) {
  TFHE_TRY(check_ctx(ctx));
  RadixShape shape;
  TFHE_TRY(check_radix_propagate(ctx, blocks_in, batch, blocks, blocks_out, &shape));
  TFHE_TRY(check_radix_reserved(ctx, batch, blocks));
  return enqueue_radix_propagate(ctx, shape, blocks_in, batch, (u32)blocks, blocks_out);
}

int tfhe_radix_propagate_batch(tfhe_context* ctx, const uint32_t* blocks_in, size_t batch, size_t blocks, uint32_t* blocks_out) {
  TFHE_TRY(check_ctx(ctx));
  RadixShape shape;
  TFHE_TRY(check_radix_propagate(ctx, blocks_in, batch, blocks, blocks_out, &shape));
  TFHE_TRY(reserve_radix(ctx, batch, blocks));
  Staging s(ctx, {batch * blocks * io_words(ctx)});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(0, blocks_in));
  TFHE_TRY(enqueue_radix_propagate(ctx, shape, s[0], batch, (u32)blocks, s[0]));
  return s.download_and_wait(0, blocks_out);
}

int tfhe_radix_compare_batch_device(tfhe_context* ctx, const uint32_t* a, const uint32_t* b, size_t batch, size_t blocks, unsigned predicate,
                                    uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  RadixShape shape;
  TFHE_TRY(check_radix_compare(ctx, a, b, batch, blocks, predicate, out, &shape));
  TFHE_TRY(check_radix_reserved(ctx, batch, blocks));
  return enqueue_radix_compare(ctx, shape, a, b, batch, (u32)blocks, predicate, out);
}

int tfhe_radix_compare_batch(tfhe_context* ctx, const uint32_t* a, const uint32_t* b, size_t batch, size_t blocks, unsigned predicate,
                             uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  RadixShape shape;
  TFHE_TRY(check_radix_compare(ctx, a, b, batch, blocks, predicate, out, &shape));
  TFHE_TRY(reserve_radix(ctx, batch, blocks));
  const size_t io = io_words(ctx);
  enum { kA, kB, kOut };
  Staging s(ctx, {batch * blocks * io, batch * blocks * io, batch * io});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kA, a));
  TFHE_TRY(s.upload(kB, b));
  TFHE_TRY(enqueue_radix_compare(ctx, shape, s[kA], s[kB], batch, (u32)blocks, predicate, s[kOut]));
  return s.download_and_wait(kOut, out);
}

int tfhe_radix_map_batch_device(tfhe_context* ctx, const uint32_t* a, size_t a_blocks, uint32_t wa, int32_t a_shift, int32_t a_fixed,
                                const uint32_t* b, size_t b_blocks, uint32_t wb, int32_t b_shift, int32_t b_fixed, size_t batch, size_t blocks,
                                const uint32_t* tables, size_t table_count, const uint32_t* table_of_block, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  const RadixMapArgs m{a, b, a_blocks, b_blocks, wa, wb, a_shift, a_fixed, b_shift, b_fixed, batch, blocks, tables, table_count, table_of_block, out};
  RadixShape shape;
  TFHE_TRY(check_radix_map(ctx, m, &shape));
  TFHE_TRY(check_radix_reserved(ctx, batch, blocks));
  return enqueue_radix_map(ctx, shape, m);
}

int tfhe_radix_map_batch(tfhe_context* ctx, const uint32_t* a, size_t a_blocks, uint32_t wa, int32_t a_shift, int32_t a_fixed,
                         const uint32_t* b, size_t b_blocks, uint32_t wb, int32_t b_shift, int32_t b_fixed, size_t batch, size_t blocks,
                         const uint32_t* tables, size_t table_count, const uint32_t* table_of_block, uint32_t* out) {
  TFHE_TRY(check_ctx(ctx));
  RadixMapArgs m{a, b, a_blocks, b_blocks, wa, wb, a_shift, a_fixed, b_shift, b_fixed, batch, blocks, tables, table_count, table_of_block, out};
  RadixShape shape;
  TFHE_TRY(check_radix_map(ctx, m, &shape));
  const size_t P = (size_t)1 << ctx->params.log_p;
  for (size_t i = 0; i < table_count * P; ++i)
    if (tables[i] >= P) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "table value >= 2^log_p");
  TFHE_TRY(reserve_radix(ctx, batch, blocks));
  const size_t io = io_words(ctx);
  enum { kA, kB, kTables, kOut };
  Staging s(ctx, {batch * a_blocks * io, b ? batch * b_blocks * io : 0, table_count * P, batch * blocks * io});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kA, a));
  if (b) TFHE_TRY(s.upload(kB, b));
  TFHE_TRY(s.upload(kTables, tables));
  m.a = s[kA], m.b = b ? s[kB] : nullptr, m.tables = s[kTables], m.out = s[kOut];
  TFHE_TRY(enqueue_radix_map(ctx, shape, m));
  return s.download_and_wait(kOut, out);
}

// ---------------------------------------------------------------------------------- on-disk format
namespace {

constexpr char kFileMagic[8] = {'T', 'F', 'H', 'E', 'A', 'M', 'D', '\1'};
constexpr size_t kFileHeaderBytes = 104;

struct FileHeader {
  u32 kind = 0, flags = 0;
  u32 params[12] = {};
  u32 ndims = 0, dims[4] = {1, 1, 1, 1};
  u64 words = 0, checksum = 0;
};

u64 fnv1a64(const unsigned char* p, size_t len, u64 h = 0xcbf29ce484222325ull) {
  for (size_t i = 0; i < len; ++i) {
    h ^= p[i];
    h *= 0x100000001b3ull;
  }
  return h;
}

void put_u32(unsigned char* p, u32 v) { for (int i = 0; i < 4; ++i) p[i] = (unsigned char)(v >> (8 * i)); }
void put_u64(unsigned char* p, u64 v) { for (int i = 0; i < 8; ++i) p[i] = (unsigned char)(v >> (8 * i)); }
u32 get_u32(const unsigned char* p) { u32 v = 0; for (int i = 0; i < 4; ++i) v |= (u32)p[i] << (8 * i); return v; }
u64 get_u64(const unsigned char* p) { u64 v = 0; for (int i = 0; i < 8; ++i) v |= (u64)p[i] << (8 * i); return v; }

void params_to_words(const tfhe_params& p, u32 out[12]) {
  const u32 w[12] = {p.glwe_dimension, p.glwe_poly_degree, p.lwe_dimension, p.padding_bits, p.log_p, p.log_q,
                     p.ks_decomposer.log_base, p.ks_decomposer.levels, p.ks_decomposer.log_q,
                     p.pbs_decomposer.log_base, p.pbs_decomposer.levels, p.pbs_decomposer.log_q};
  std::memcpy(out, w, sizeof(w));
}

void words_to_params(const u32 w[12], tfhe_params* p) {
  p->glwe_dimension = w[0];
  p->glwe_poly_degree = w[1];
  p->lwe_dimension = w[2];
  p->padding_bits = w[3];
  p->log_p = w[4];
  p->log_q = w[5];
  p->ks_decomposer = {w[6], w[7], w[8]};
  p->pbs_decomposer = {w[9], w[10], w[11]};
}

int read_header(std::FILE* f, FileHeader* h) {
  unsigned char b[kFileHeaderBytes];
  if (std::fread(b, 1, sizeof(b), f) != sizeof(b)) return TFHE_ERR_IO;
  if (std::memcmp(b, kFileMagic, 8) != 0) return TFHE_ERR_IO;
  h->kind = get_u32(b + 8);
  h->flags = get_u32(b + 12);
  for (int i = 0; i < 12; ++i) h->params[i] = get_u32(b + 16 + 4 * i);
  h->ndims = get_u32(b + 64);
  for (int i = 0; i < 4; ++i) h->dims[i] = get_u32(b + 68 + 4 * i);
  h->words = get_u64(b + 88);
  h->checksum = get_u64(b + 96);
  if (h->kind < TFHE_FILE_BSK || h->kind > TFHE_FILE_PKSK || h->ndims == 0 || h->ndims > 4) return TFHE_ERR_IO;
  u64 prod = 1;
  for (u32 i = 0; i < 4; ++i) {
    if (h->dims[i] == 0 || (i >= h->ndims && h->dims[i] != 1)) return TFHE_ERR_IO;
    if (prod > (~0ull) / h->dims[i]) return TFHE_ERR_IO;
    prod *= h->dims[i];
  }
  if (prod != h->words) return TFHE_ERR_IO;
  // words * 4 + header must not wrap (a crafted header with words = 2^62 would otherwise pass the
  // size check below as 0 and make the caller allocate from attacker-chosen dims)
  if (h->words > ((u64)SIZE_MAX - kFileHeaderBytes) / sizeof(u32)) return TFHE_ERR_IO;
  return TFHE_OK;
}

}  // namespace

int tfhe_file_write(const char* path, uint32_t kind, const tfhe_params* params, uint32_t flags,
                    const uint32_t* dims, uint32_t ndims, const uint32_t* data) {
  if (!path || !params || !dims || !data || ndims == 0 || ndims > 4 || kind < TFHE_FILE_BSK || kind > TFHE_FILE_PKSK)
    return TFHE_ERR_INVALID_ARGUMENT;
  u64 words = 1;
  for (u32 i = 0; i < ndims; ++i) {
    if (dims[i] == 0 || words > (~0ull) / dims[i]) return TFHE_ERR_INVALID_ARGUMENT;
    words *= dims[i];
  }
  unsigned char b[kFileHeaderBytes] = {};
  std::memcpy(b, kFileMagic, 8);
  put_u32(b + 8, kind);
  put_u32(b + 12, flags);
  u32 pw[12];
  params_to_words(*params, pw);
  for (int i = 0; i < 12; ++i) put_u32(b + 16 + 4 * i, pw[i]);
  put_u32(b + 64, ndims);
  for (u32 i = 0; i < 4; ++i) put_u32(b + 68 + 4 * i, i < ndims ? dims[i] : 1u);
  put_u64(b + 88, words);
  // payload is written as little-endian u32 words; this library only targets little-endian hosts,
  // so the in-memory bytes are the file bytes
  put_u64(b + 96, fnv1a64(reinterpret_cast<const unsigned char*>(data), (size_t)words * sizeof(u32)));
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return TFHE_ERR_IO;
  bool ok = std::fwrite(b, 1, sizeof(b), f) == sizeof(b) &&
            std::fwrite(data, sizeof(u32), (size_t)words, f) == (size_t)words;
  ok = (std::fclose(f) == 0) && ok;
  return ok ? TFHE_OK : TFHE_ERR_IO;
}

int tfhe_file_read_header(const char* path, uint32_t* kind, tfhe_params* params, uint32_t* flags,
                          uint32_t dims[4], uint32_t* ndims, uint64_t* words) {
  if (!path) return TFHE_ERR_INVALID_ARGUMENT;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return TFHE_ERR_IO;
  FileHeader h;
  int st = read_header(f, &h);
  if (st == TFHE_OK) {  // the payload must be all there, and nothing after it
    if (std::fseek(f, 0, SEEK_END) != 0) st = TFHE_ERR_IO;
    const long end = std::ftell(f);
    if (end < 0 || (u64)end != kFileHeaderBytes + h.words * sizeof(u32)) st = TFHE_ERR_IO;
  }
  std::fclose(f);
  if (st) return st;
  if (kind) *kind = h.kind;
  if (params) words_to_params(h.params, params);
  if (flags) *flags = h.flags;
  if (dims) std::memcpy(dims, h.dims, sizeof(h.dims));
  if (ndims) *ndims = h.ndims;
  if (words) *words = h.words;
  return TFHE_OK;
}

int tfhe_file_read(const char* path, uint32_t* data, uint64_t words) {
  if (!path || !data) return TFHE_ERR_INVALID_ARGUMENT;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return TFHE_ERR_IO;
  FileHeader h;
  int st = read_header(f, &h);
  if (st == TFHE_OK && h.words != words) st = TFHE_ERR_INVALID_ARGUMENT;
  if (st == TFHE_OK && std::fread(data, sizeof(u32), (size_t)words, f) != (size_t)words) st = TFHE_ERR_IO;
  unsigned char extra;
  if (st == TFHE_OK && std::fread(&extra, 1, 1, f) != 0) st = TFHE_ERR_IO;
  std::fclose(f);
  if (st == TFHE_OK &&
      fnv1a64(reinterpret_cast<const unsigned char*>(data), (size_t)words * sizeof(u32)) != h.checksum)
    st = TFHE_ERR_IO;
  return st;
}

// ---------------------------------------------------------------------------------- test vectors / gates
int tfhe_construct_test_from_lut(const tfhe_params* params, const uint32_t* lut, size_t lut_len, uint32_t* out) {
  if (!params || !lut || !out) return TFHE_ERR_INVALID_ARGUMENT;
  int st = tfhe_params_validate(params);
  if (st) return st;
  return test_from_lut(params, lut, lut_len, out);
}

int tfhe_construct_test_vector_boolean(const tfhe_params* params, const uint32_t truth[4], uint32_t* out) {
  if (!params || !truth || !out) return TFHE_ERR_INVALID_ARGUMENT;
  int st = tfhe_params_validate(params);
  if (st) return st;
  const u32 pm = 1u << params->log_p;
  std::vector<u32> lut(pm);
  for (u32 i = 0; i < pm; ++i) lut[i] = truth[(((i >> 1) & 1u) << 1) | (i & 1u)];  // test_vector.rs:16
  return test_from_lut(params, lut.data(), pm, out);
}

// notes/Boolean Gates.md:2-11: a gate of m inputs is one PBS of c_in = sum_i 2^i * cts[i] with the
// test vector of lut[x] = truth[x mod 2^m]; and()/or() (boolean.rs:9-53) are the m = 2 case.
static int lut_gate_device(tfhe_context* ctx, const u32* truth, u32 inputs, const u32* const* cts,
                           size_t batch, u32* lwe_out) {
  TFHE_TRY(check_present(ctx, {truth, cts, lwe_out}, batch));
  if (inputs == 0 || inputs > ctx->params.log_p || inputs > 8)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "gate inputs must be 1..min(log_p, 8): the plaintext space holds log_p bits");
  for (u32 i = 0; i < inputs; ++i)
    if (!cts[i]) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null input ciphertext");
  if (!ctx->have_key) return fail(ctx, TFHE_ERR_NO_KEY, "load the bootstrapping key first");
  TFHE_TRY(reserve(ctx, batch));
  const size_t words = batch * io_words(ctx);
  const u32 entries = 1u << inputs;
  tfhe_context::GateTv* slot = nullptr;
  for (auto& g : ctx->gate_tvs)
    if (g.truth.size() == entries && std::memcmp(g.truth.data(), truth, entries * sizeof(u32)) == 0) slot = &g;
  // A captured graph keeps slot->d_tv and its replays never come back here, so a table looked up during a capture is
  // pinned: its buffer is not handed to another table.  (A failed query is read as a capture, as the blind rotation's fork reads it.)
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(ctx->stream, &capture) != hipSuccess || capture != hipStreamCaptureStatusNone;
  if (!slot) {
    // first use of this truth table: build its test vector on the host and upload it (this one
    // call synchronises; later calls with a table already seen do not).  At most kMaxGateTvs
    // unpinned tables are kept; the least recently used of them is replaced.
    if (capturing)
      return fail(ctx, TFHE_ERR_INVALID_ARGUMENT,
                  "first use of this truth table during a stream capture: its upload synchronises, run the gate once before capturing");
    const u32 pm = 1u << ctx->params.log_p;
    std::vector<u32> lut(pm), tv(ctx->N);
    for (u32 x = 0; x < pm; ++x) lut[x] = truth[x & (entries - 1)];  // test_vector.rs:16 for m = 2
    if (int st = test_from_lut(&ctx->params, lut.data(), pm, tv.data()))
      return fail(ctx, st, "truth table / plaintext space mismatch");
    TFHE_TRY(check_tv_host(ctx, tv.data(), ctx->N));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    size_t unpinned = 0;
    for (auto& g : ctx->gate_tvs) {
      if (g.pinned) continue;
      ++unpinned;
      if (!slot || g.last_use < slot->last_use) slot = &g;  // the victim, if one is needed
    }
    if (unpinned < tfhe_context::kMaxGateTvs) {  // room left, or every entry is pinned: the cache grows
      ctx->gate_tvs.emplace_back();
      slot = &ctx->gate_tvs.back();
      TFHE_TRY(slot->d_tv.grow(ctx, ctx->N * sizeof(u32)));
    }
    slot->truth.clear();  // not a valid entry until the upload has succeeded
    HIP_TRY(ctx, hipMemcpy(slot->d_tv.as(), tv.data(), ctx->N * sizeof(u32), hipMemcpyHostToDevice));
    slot->truth.assign(truth, truth + entries);
  }
  slot->last_use = ++ctx->gate_clock;
  if (capturing) slot->pinned = true;
  const u32* d_in = cts[0];
  for (u32 i = 1; i < inputs; ++i) {  // 2*ct1 + ct0 (boolean.rs:18), then + 4*ct2, ...
    HIP_TRY(ctx, launch::lwe_linear(ctx->stream, 1u, d_in, 1u << i, cts[i], words, ctx->d_lwe_in2.as<u32>()));
    d_in = ctx->d_lwe_in2.as<u32>();
  }
  return enqueue_bootstrap(ctx, d_in, batch, slot->d_tv.as<u32>(), 1, ctx->d_lwe_big.as<u32>(), lwe_out);
}

int tfhe_gate_batch_device(tfhe_context* ctx, const uint32_t truth[4], const uint32_t* ct0,
                           const uint32_t* ct1, size_t batch, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  if (!ct0 || !ct1) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer / empty batch");
  const u32* cts[2] = {ct0, ct1};
  return lut_gate_device(ctx, truth, 2, cts, batch, lwe_out);
}

int tfhe_lut_gate_batch_device(tfhe_context* ctx, const uint32_t* truth, uint32_t inputs,
                               const uint32_t* const* cts, size_t batch, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  return lut_gate_device(ctx, truth, inputs, cts, batch, lwe_out);
}

int tfhe_lut_gate_batch(tfhe_context* ctx, const uint32_t* truth, uint32_t inputs, const uint32_t* const* cts,
                        size_t batch, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  if (!truth || !cts || !lwe_out || batch == 0 || inputs == 0 || inputs > 8)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer / empty batch / bad input count");
  Staging s(ctx, std::vector<size_t>(inputs + 1, batch * io_words(ctx)));  // the inputs, then the result
  TFHE_TRY(s.reserve());
  const u32* d_cts[8];
  for (u32 i = 0; i < inputs; ++i) {
    if (!cts[i]) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null input ciphertext");
    TFHE_TRY(s.upload(i, cts[i]));
    d_cts[i] = s[i];
  }
  TFHE_TRY(lut_gate_device(ctx, truth, inputs, d_cts, batch, s[inputs]));
  return s.download_and_wait(inputs, lwe_out);
}

int tfhe_gate_batch(tfhe_context* ctx, const uint32_t truth[4], const uint32_t* ct0,
                    const uint32_t* ct1, size_t batch, uint32_t* lwe_out) {
  const uint32_t* cts[2] = {ct0, ct1};
  if (!ct0 || !ct1) return ctx ? fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null pointer / empty batch") : TFHE_ERR_INVALID_ARGUMENT;
  return tfhe_lut_gate_batch(ctx, truth, 2, cts, batch, lwe_out);
}

// NOT needs no bootstrap: an encryption of 1 - m is (-a, enc(1) - b), enc(1) = 1 << (32 - log_p - padding)
int tfhe_lwe_not_batch_device(tfhe_context* ctx, const uint32_t* ct, size_t batch, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {ct, lwe_out}, batch));
  const size_t n1 = io_words(ctx);
  const u32 one = 1u << (32 - ctx->params.log_p - ctx->params.padding_bits);
  HIP_TRY(ctx, launch::lwe_linear(ctx->stream, 0xFFFFFFFFu, ct, 0u, nullptr, batch * n1, lwe_out, n1, one));
  return TFHE_OK;
}

int tfhe_lwe_not_batch(tfhe_context* ctx, const uint32_t* ct, size_t batch, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  TFHE_TRY(check_present(ctx, {ct, lwe_out}, batch));
  enum { kIn, kOut };
  Staging s(ctx, {batch * io_words(ctx), batch * io_words(ctx)});
  TFHE_TRY(s.reserve());
  TFHE_TRY(s.upload(kIn, ct));
  TFHE_TRY(tfhe_lwe_not_batch_device(ctx, s[kIn], batch, s[kOut]));
  return s.download_and_wait(kOut, lwe_out);
}

// ---------------------------------------------------------------------------------- seeded ciphertexts
// include/tfhe_hip.h ("seeded ciphertexts") states the generator and the two layouts; seeded.h the launches.
namespace {

SeededStream seeded_stream(const tfhe_seed* seed, u32 domain) {
  SeededStream s;
  for (int i = 0; i < 8; ++i) s.key[i] = seed->key[i];
  s.nonce[0] = domain, s.nonce[1] = (u32)seed->stream, s.nonce[2] = (u32)(seed->stream >> 32);
  return s;
}

bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

// rows of mask_words mask words and 2^body_shift body words: the one shape behind both layouts
struct SeededShape {
  size_t mask_words;
  u32 body_shift;
  u32 domain;
  size_t body_words() const { return (size_t)1 << body_shift; }
  size_t row_words() const { return mask_words + body_words(); }
};
SeededShape lwe_shape(size_t dimension) { return {dimension, 0, TFHE_SEED_DOMAIN_LWE}; }
SeededShape glwe_shape(const tfhe_context* ctx) { return {(size_t)ctx->big_n, ctx->pbs.log_n, TFHE_SEED_DOMAIN_GLWE}; }

// every refusal of an expansion; *first_word = first_row * mask_words
int check_expand(tfhe_context* ctx, const tfhe_seed* seed, const u32* bodies, u64 first_row, size_t rows, const SeededShape& sh,
                 const u32* out, u64* first_word) {
  if (!seed || !out) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null seed or output");
  if (rows == 0 || sh.mask_words == 0 || sh.mask_words >= ((size_t)1 << 31))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "no rows, or a dimension that is zero or 2^31 and above");
  const u64 max_rows = kSeededMaxWords / sh.mask_words;
  if (rows > max_rows || first_row > max_rows - rows)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the word range (first_row + rows) * dimension reaches past TFHE_SEED_MAX_WORDS = 2^36");
  if (bodies && ranges_overlap(bodies, rows * sh.body_words() * sizeof(u32), out, rows * sh.row_words() * sizeof(u32)))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "bodies and the output overlap");
  *first_word = first_row * sh.mask_words;
  return TFHE_OK;
}

int check_compress(tfhe_context* ctx, const u32* in, size_t rows, const SeededShape& sh, const u32* out) {
  if (!in || !out) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null input or output");
  if (rows == 0 || sh.mask_words == 0 || sh.mask_words >= ((size_t)1 << 31) || rows > kSeededMaxWords / sh.mask_words)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "no rows, a dimension that is zero or 2^31 and above, or more than 2^36 mask words");
  if (ranges_overlap(in, rows * sh.row_words() * sizeof(u32), out, rows * sh.body_words() * sizeof(u32)))
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the input and the output overlap");
  return TFHE_OK;
}

int expand_device(tfhe_context* ctx, const tfhe_seed* seed, const u32* bodies, u64 first_row, size_t rows, const SeededShape& sh, u32* out) {
  u64 first_word = 0;
  TFHE_TRY(check_expand(ctx, seed, bodies, first_row, rows, sh, out, &first_word));
  const SeededRowsArgs a{seeded_stream(seed, sh.domain), bodies, out, first_word, rows, (u32)sh.mask_words, sh.body_shift};
  HIP_TRY(ctx, launch::seeded_expand(ctx->stream, a));
  return TFHE_OK;
}

// bodies go up (or, without bodies, the rows themselves: their body words stay), the rows come back
int expand_host(tfhe_context* ctx, const tfhe_seed* seed, const u32* bodies, u64 first_row, size_t rows, const SeededShape& sh, u32* out) {
  u64 first_word = 0;
  TFHE_TRY(check_expand(ctx, seed, bodies, first_row, rows, sh, out, &first_word));
  enum { kBodies, kRows };
  Staging s(ctx, {(rows * sh.body_words() + 3) & ~(size_t)3, rows * sh.row_words()});
  TFHE_TRY(s.reserve());
  if (bodies)
    TFHE_TRY(upload(ctx, s[kBodies], bodies, rows * sh.body_words()));
  else
    TFHE_TRY(s.upload(kRows, out));
  TFHE_TRY(expand_device(ctx, seed, bodies ? s[kBodies] : nullptr, first_row, rows, sh, s[kRows]));
  return s.download_and_wait(kRows, out);
}

int compress_device(tfhe_context* ctx, const u32* in, size_t rows, const SeededShape& sh, u32* out) {
  TFHE_TRY(check_compress(ctx, in, rows, sh, out));
  const SeededRowsArgs a{SeededStream{}, in, out, 0, rows, (u32)sh.mask_words, sh.body_shift};
  HIP_TRY(ctx, launch::seeded_compress(ctx->stream, a));
  return TFHE_OK;
}

int compress_host(tfhe_context* ctx, const u32* in, size_t rows, const SeededShape& sh, u32* out) {
  TFHE_TRY(check_compress(ctx, in, rows, sh, out));
  enum { kRows, kBodies };
  Staging s(ctx, {(rows * sh.row_words() + 3) & ~(size_t)3, rows * sh.body_words()});
  TFHE_TRY(s.reserve());
  TFHE_TRY(upload(ctx, s[kRows], in, rows * sh.row_words()));
  TFHE_TRY(compress_device(ctx, s[kRows], rows, sh, s[kBodies]));
  return s.download_and_wait(kBodies, out);
}

}  // namespace

int tfhe_seed_words(const tfhe_seed* seed, uint32_t domain, uint64_t first_word, size_t count, uint32_t* out) {
  if (first_word > kSeededMaxWords || count > kSeededMaxWords - first_word) return TFHE_ERR_INVALID_ARGUMENT;
  if (count == 0) return TFHE_OK;
  if (!seed || !out) return TFHE_ERR_INVALID_ARGUMENT;
  const SeededStream s = seeded_stream(seed, domain);
  u32 x[16];
  u64 w = first_word;
  const u64 end = first_word + count;
  while (w < end) {
    seeded_block(s, (u32)(w / kSeededBlockWords), x);
    for (u32 i = (u32)(w % kSeededBlockWords); i < kSeededBlockWords && w < end; ++i, ++w) out[w - first_word] = x[i];
  }
  return TFHE_OK;
}

int tfhe_expand_lwe_rows_device(tfhe_context* ctx, const tfhe_seed* seed, const uint32_t* bodies, uint64_t first_row, size_t rows,
                                size_t dimension, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  return expand_device(ctx, seed, bodies, first_row, rows, lwe_shape(dimension), lwe_out);
}

int tfhe_expand_lwe_rows(tfhe_context* ctx, const tfhe_seed* seed, const uint32_t* bodies, uint64_t first_row, size_t rows,
                         size_t dimension, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  return expand_host(ctx, seed, bodies, first_row, rows, lwe_shape(dimension), lwe_out);
}

int tfhe_expand_glwe_rows_device(tfhe_context* ctx, const tfhe_seed* seed, const uint32_t* bodies, uint64_t first_row, size_t rows,
                                 uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  return expand_device(ctx, seed, bodies, first_row, rows, glwe_shape(ctx), glwe_out);
}

int tfhe_expand_glwe_rows(tfhe_context* ctx, const tfhe_seed* seed, const uint32_t* bodies, uint64_t first_row, size_t rows,
                          uint32_t* glwe_out) {
  TFHE_TRY(check_ctx(ctx));
  return expand_host(ctx, seed, bodies, first_row, rows, glwe_shape(ctx), glwe_out);
}

int tfhe_compress_lwe_rows_device(tfhe_context* ctx, const uint32_t* lwe, size_t rows, size_t dimension, uint32_t* bodies_out) {
  TFHE_TRY(check_ctx(ctx));
  return compress_device(ctx, lwe, rows, lwe_shape(dimension), bodies_out);
}

int tfhe_compress_lwe_rows(tfhe_context* ctx, const uint32_t* lwe, size_t rows, size_t dimension, uint32_t* bodies_out) {
  TFHE_TRY(check_ctx(ctx));
  return compress_host(ctx, lwe, rows, lwe_shape(dimension), bodies_out);
}

int tfhe_compress_glwe_rows_device(tfhe_context* ctx, const uint32_t* glwe, size_t rows, uint32_t* bodies_out) {
  TFHE_TRY(check_ctx(ctx));
  return compress_device(ctx, glwe, rows, glwe_shape(ctx), bodies_out);
}

int tfhe_compress_glwe_rows(tfhe_context* ctx, const uint32_t* glwe, size_t rows, uint32_t* bodies_out) {
  TFHE_TRY(check_ctx(ctx));
  return compress_host(ctx, glwe, rows, glwe_shape(ctx), bodies_out);
}

int tfhe_load_bootstrapping_key_seeded(tfhe_context* ctx, const tfhe_seed* bsk_seed, const uint32_t* bsk_bodies,
                                       const tfhe_seed* ksk_seed, const uint32_t* ksk_bodies) {
  TFHE_TRY(check_ctx(ctx));
  if (!bsk_seed || !bsk_bodies || !ksk_seed || !ksk_bodies) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null seed or key pointer");
  const size_t n = ctx->params.lwe_dimension;
  const size_t bsk_rows = n * ctx->R, bsk_body_words = bsk_rows * ctx->N, ksk_rows = (size_t)ctx->big_n * ctx->ks.levels;
  // bodies, then the raw arrays: temporaries of this call (the device loader drains the stream before it returns)
  DeviceBuffer bodies, raw_bsk, raw_ksk;
  TFHE_TRY(bodies.grow(ctx, (bsk_body_words + ksk_rows) * sizeof(u32)));
  TFHE_TRY(raw_bsk.grow(ctx, bsk_rows * glwe_words(ctx) * sizeof(u32)));
  TFHE_TRY(raw_ksk.grow(ctx, ksk_words(ctx) * sizeof(u32)));
  TFHE_TRY(upload(ctx, bodies.as<u32>(), bsk_bodies, bsk_body_words));
  TFHE_TRY(upload(ctx, bodies.as<u32>() + bsk_body_words, ksk_bodies, ksk_rows));
  int st = expand_device(ctx, bsk_seed, bodies.as<u32>(), 0, bsk_rows, glwe_shape(ctx), raw_bsk.as<u32>());
  if (st == TFHE_OK) st = expand_device(ctx, ksk_seed, bodies.as<u32>() + bsk_body_words, 0, ksk_rows, lwe_shape(n), raw_ksk.as<u32>());
  if (st == TFHE_OK) st = tfhe_load_bootstrapping_key_device(ctx, raw_bsk.as<u32>(), raw_ksk.as<u32>());
  // the temporaries are freed on return: whatever was enqueued on them ends first, also after a failure
  const hipError_t drained = hipStreamSynchronize(ctx->stream);
  if (st == TFHE_OK && drained != hipSuccess) return hip_fail(ctx, drained, "hipStreamSynchronize");
  return st;
}

int tfhe_bootstrap_batch_seeded(tfhe_context* ctx, const tfhe_seed* seed, uint64_t first_row, const uint32_t* bodies, size_t batch,
                                const uint32_t* tv, size_t tv_count, uint32_t* lwe_out) {
  TFHE_TRY(check_ctx(ctx));
  if (!seed) return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "null seed");
  TFHE_TRY(check_rotate_args(ctx, bodies, tv, lwe_out, batch, tv_count));
  TFHE_TRY(check_tv_host(ctx, tv, tv_count * ctx->N));
  const SeededShape sh = lwe_shape(io_words(ctx) - 1);
  const u64 max_rows = kSeededMaxWords / sh.mask_words;
  if (batch > max_rows || first_row > max_rows - batch)
    return fail(ctx, TFHE_ERR_INVALID_ARGUMENT, "the word range (first_row + batch) * dimension reaches past TFHE_SEED_MAX_WORDS = 2^36");
  TFHE_TRY(reserve(ctx, batch));
  // the bodies wait in the second operand's buffer, the expanded rows are the first operand
  TFHE_TRY(upload(ctx, ctx->d_lwe_in2.as<u32>(), bodies, batch));
  TFHE_TRY(upload(ctx, ctx->d_tv.as<u32>(), tv, tv_count * ctx->N));
  TFHE_TRY(expand_device(ctx, seed, ctx->d_lwe_in2.as<u32>(), first_row, batch, sh, ctx->d_lwe_in.as<u32>()));
  TFHE_TRY(enqueue_bootstrap(ctx, ctx->d_lwe_in.as<u32>(), batch, ctx->d_tv.as<u32>(), tv_count, ctx->d_lwe_big.as<u32>(), ctx->d_lwe_out.as<u32>()));
  return download_and_wait(ctx, lwe_out, ctx->d_lwe_out.as<u32>(), batch * io_words(ctx));
}

}  // extern "C"
