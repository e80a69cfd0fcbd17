// context.h -- the state behind a tfhe_context handle, shared by the host-side sources of the library
// (capi.cpp: the single-device C ABI; pool.cpp: the multi-device pool built on top of it).  Private to csrc/.
#pragma once
#include "tfhe_hip.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "launch.h"

using namespace tfhe;

// A device allocation that its holder owns: every workspace, key buffer and temporary of the host sources is one.  The
// destructor frees it (with its device current: tfhe_context_destroy and tfhe_poly_weights_destroy select it first).
// The size changes in two ways only, grow and resize, and both keep ONE rule: the buffer never claims a capacity it
// does not have.  They drain ctx->stream (work enqueued on the old allocation ends first), read as null with capacity
// 0 from before the old allocation is freed, and record the new capacity only after the new allocation succeeded --
// so after any failure the buffer is null, capacity 0, and a later, smaller call is refused or allocates again
// instead of launching kernels on memory that is gone.  An owner's logical sizes (ws_batch, mv_batch, ..) follow the
// same discipline around the call: zeroed before, set after.
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : ptr_(o.ptr_), bytes_(o.bytes_) {
    o.ptr_ = nullptr;
    o.bytes_ = 0;
  }
  ~DeviceBuffer() {
    if (ptr_) (void)hipFree(ptr_);
  }
  template <class T = void>
  T* as() const { return static_cast<T*>(ptr_); }
  explicit operator bool() const { return ptr_ != nullptr; }
  size_t bytes() const { return bytes_; }
  size_t words() const { return bytes_ / sizeof(u32); }
  // at least `bytes`: nothing happens (no HIP call) when the capacity covers them; never shrinks
  int grow(tfhe_context* ctx, size_t bytes) { return bytes <= bytes_ ? TFHE_OK : reallocate(ctx, bytes); }
  // exactly `bytes` (0: released): the prepared keys, whose footprint follows the kind and dimension of the loaded key
  int resize(tfhe_context* ctx, size_t bytes) { return bytes == bytes_ ? TFHE_OK : reallocate(ctx, bytes); }

 private:
  int reallocate(tfhe_context* ctx, size_t bytes);  // below, after tfhe_context
  void* ptr_ = nullptr;
  size_t bytes_ = 0;
};

struct tfhe_context {
  tfhe_params params;
  PbsParams pbs;
  KsParams ks;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  launch::SideStream side = {nullptr, nullptr, nullptr};  // the blind rotation's second stream (always the context's own)
  u32 N = 0, R = 0, big_n = 0;

  int field = 0;              // launch::kFieldGoldilocks | launch::kFieldFp64
  int parts = 1;              // spectra per key polynomial in this field
  DeviceBuffer d_tw;          // psi_rev[N], 8-byte field elements
  DeviceBuffer d_queue;       // ticket counter of the external-product kernel's work queue (unsigned long long)
  DeviceBuffer d_bsk;         // prepared BSK [n][R][k+1][parts][N] (spectrum_slot order, x 1/N)
  DeviceBuffer d_ksk;         // [big_n*l_ks][n+1]
  DeviceBuffer d_ksk_matrix;  // the same key in the matrix path's layout (ks_matrix.h); null where it is not admitted
  int ks_path = 0;            // path of the key switch (tfhe_context_set_key_switch_path): launch::kKsPath*
  bool have_key = false;
  bool bmmp = false;          // the loaded key is a BMMP key: n/2 * 3 GGSWs (tfhe_load_bootstrapping_key_bmmp)
  size_t bsk_ggsws = 0;       // GGSWs d_bsk was allocated for
  // packing key (tfhe_load_packing_key): independent of the bootstrapping key
  DeviceBuffer d_pksk;        // prepared: ceil(pksk_dim / (k+1)) slices of [(k+1) l_ks][k+1][parts][N], zero-filled past pksk_dim
  size_t pksk_dim = 0;        // dimension of the LWE key it packs from
  bool have_pksk = false;
  DeviceBuffer d_pack_cols;   // transposed inputs of a packing call, kPackColsWords words (capi.cpp) or one output's worth
  // CMUX tree / table lookup (tfhe_context_reserve_lookup): partial results of the passes and the teams' pending slots
  DeviceBuffer d_lookup_ws;
  unsigned lookup_height = 0; // subtree height a team reduces (tfhe_context_set_lookup_subtree_height); 0: automatic
  // DEMUX tree / table update (tfhe_context_reserve_demux): the passes' nodes and the teams' parked nodes
  DeviceBuffer d_demux_ws;
  unsigned demux_height = 0;  // subtree height a team expands (tfhe_context_set_demux_subtree_height); 0: automatic
  // Encrypted branching program (tfhe_context_reserve_program): one buffer, [values: one GLWE per (query, node)] then
  // kProgramImages images of program_image_words words each -- a program compiled for the device (its ops in execution
  // order, then its outputs).  An image is uploaded on the first use of a program (that call synchronises; a program
  // already resident costs a comparison on the host) and the least recently used unpinned one is replaced.  As with
  // gate_tvs below, an image used while the stream is capturing is pinned: the graph holds its address.  Reserving
  // again un-pins and forgets all images (the buffer may have moved: graphs captured before are void).
  static constexpr size_t kProgramImages = 4;
  struct ProgramImage {
    std::vector<u32> key;            // n_inputs, n_terminals, n_nodes, n_outputs, the nodes, the outputs; empty: free
    std::vector<u32> level_counts;   // nodes per dependency level, in execution order
    unsigned long long last_use = 0;
    bool pinned = false;
  };
  DeviceBuffer d_program_ws;
  size_t program_value_words = 0, program_image_words = 0;
  ProgramImage program_images[kProgramImages];
  unsigned long long program_clock = 0;
  unsigned program_parts = 0;  // teams per query of a split level (tfhe_context_set_program_split); 0: automatic
  // Dense layer (tfhe_context_reserve_dense): the fused layer's pre-activations [dense_rows][max(n, k N) + 1], then one
  // test vector [N] per bootstrap, for dense_rows = max_queries * max_outputs bootstraps
  DeviceBuffer d_dense_ws;
  size_t dense_rows = 0;
  unsigned dense_parts = 0;   // shares of the inputs (tfhe_context_set_dense_split); 0: automatic
  // Encrypted convolution (tfhe_context_reserve_glwe_conv): the prepared spectra of a call's ciphertext polynomials,
  // conv_ws_polys = max_queries * max_channels * (k+1) of them, parts * N 8-byte words each
  DeviceBuffer d_conv_ws;
  size_t conv_ws_polys = 0;
  unsigned conv_rows = 0;     // channels per pass (tfhe_context_set_glwe_conv_rows); 0: automatic
  // tree LUT (tfhe_context_reserve_tree_lut): per-rotation inputs, segment state, the levels' results and packed GLWEs
  DeviceBuffer d_tree_ws;
  // digit extraction (tfhe_context_reserve_extract): the remainder r, the scaled input s and the result o of the bit's
  // bootstrap, each [extract_batch][max(n, k N) + 1], the shared constant accumulator [k+1][N], then extract_digits digit
  // buffers of the same rows (the host forms' and the wide LUT's digits)
  DeviceBuffer d_extract_ws;
  size_t extract_batch = 0, extract_digits = 0;
  // radix integers (tfhe_context_reserve_radix).  With R = 2 radix_batch radix_blocks rotations and rows of
  // max(n, k N) + 1 words: a level's inputs x [R], level 1's results o [R], the sums w [R / 2] and the states s [R / 2],
  // all [block][row] between two levels, then a level's accumulators [R][k+1][N].  d_radix_tables: the fixed tables
  // [kRadixTables][2^log_p] (radix.h::RadixTable), written once by the first reservation.
  DeviceBuffer d_radix_ws;
  DeviceBuffer d_radix_tables;
  size_t radix_batch = 0, radix_blocks = 0;
  // multi-value bootstrap.  d_mv_const (allocated by tfhe_context_reserve_multi_value, by tfhe_context_set_tree_lut_level0(1)
  // and by the host forms): the constant accumulator (0, .., 0, kappa (1 + X + .. + X^(N-1))) [k+1][N], the B + 1 positions
  // of a lookup table's coefficients [kSparseMaxTerms], a caller's positions [kSparseMaxTerms].  d_mv_ws
  // (tfhe_context_reserve_multi_value): the key-switched inputs [mv_batch][n + 1], the rotated accumulators
  // [mv_batch][k+1][N], the coefficients [mv_batch][mv_tables][B + 1], the combinations before the key switch
  // [mv_batch][mv_tables][k N + 1]
  DeviceBuffer d_mv_const;
  DeviceBuffer d_mv_ws;
  size_t mv_batch = 0, mv_tables = 0;
  bool tree_level0_multi_value = false;  // tfhe_context_set_tree_lut_level0
  // multi-bit blind rotation (tfhe_context_reserve_multibit): the bundles of one call, per sample ceil(n / g) prepared GGSWs
  DeviceBuffer d_mb_ws;
  // block-binary blind rotation (block_rotate.h): the factors zeta^e - 1, e in [0, 2N); made with the context where the
  // rotation is offered, empty elsewhere
  DeviceBuffer d_block_roots;
  bool aligned = false;       // decomposer alignment (tfhe_context_set_decomposer_alignment)
  bool ks_first = false;      // bootstrap order (tfhe_context_set_bootstrap_order)
  int shape = 0;              // kernel shape of the blind rotation (tfhe_context_set_kernel_shape): launch::kShape*

  // workspace (grown on demand by host-pointer calls or tfhe_context_reserve)
  size_t ws_batch = 0;
  DeviceBuffer d_lwe_in;      // [batch][n+1]
  DeviceBuffer d_lwe_in2;     // [batch][n+1] second gate operand
  DeviceBuffer d_lwe_big;     // [batch][big_n+1]
  DeviceBuffer d_lwe_out;     // [batch][n+1]
  DeviceBuffer d_lwe_ks;      // [batch][n+1] key-switched input of the KS-then-PBS order
  DeviceBuffer d_glwe_a;      // [batch][k+1][N]
  DeviceBuffer d_glwe_b;
  DeviceBuffer d_glwe_c;
  DeviceBuffer d_tv;          // [batch][N] (or [1][N])
  // test vectors of gate calls, one [N] device buffer per truth table seen (a gate graph alternates
  // between a handful of tables; re-uploading on every switch would synchronise the stream).  kMaxGateTvs unpinned
  // tables are kept, the least recently used one is replaced.  A table looked up while the stream is capturing is
  // pinned for the life of the context: the captured graph holds d_tv, a replay does not pass through the cache, so
  // that buffer is never rewritten with another table (pinned entries do not count towards the limit).
  static constexpr size_t kMaxGateTvs = 64;
  struct GateTv {
    std::vector<u32> truth;  // 2^inputs entries
    DeviceBuffer d_tv;
    unsigned long long last_use = 0;
    bool pinned = false;
  };
  std::vector<GateTv> gate_tvs;
  unsigned long long gate_clock = 0;
  // generic scratch for the small entry points
  DeviceBuffer d_misc;
  DeviceBuffer d_ggsw_tmp;    // prepared GGSWs of external_product / cmux host calls (8-byte words)
  DeviceBuffer d_ggsw_raw;
  DeviceBuffer d_key_tmp;     // secret keys / messages of the encryption-side calls

  bool timing = false;
  // br start/stop, ks start/stop of the current timing slot.  Bootstraps rotate through kTimingSlots sets of
  // events, so that a caller can time K back-to-back steps without a host synchronisation inside the loop and
  // read them all afterwards (tfhe_kernel_ms_ago); the other timed calls use the current set.
  static constexpr int kTimingSlots = 64;
  hipEvent_t ev_ring[kTimingSlots][4] = {};
  hipEvent_t* ev = ev_ring[0];
  int ev_slot = 0;
  unsigned long long timed_bootstraps = 0;
  bool ev_valid_br = false, ev_valid_ks = false;
  bool ev_valid_mb = false;  // the current slot's events bracket a multi-bit rotation's two launches (tfhe_multibit_last_kernel_ms)

  std::string last_error;
};

// A prepared set of clear weight polynomials (tfhe_prepare_poly_weights): the transformed polynomials on the device of
// the context that prepared them, for that context's backend and ring.
struct tfhe_poly_weights {
  int device = 0;
  int field = 0;
  u32 log_n = 0;
  DeviceBuffer d_spec;         // [outputs][channels] spectra, N 8-byte words each (glwe_conv.h::conv_weights_wave)
  size_t outputs = 0, channels = 0;
  unsigned weight_bits = 0;    // the smallest b with every |w| <= 2^b
  unsigned rows_per_pass = 0;  // channels the backend's exactness rule admits in one pass at that magnitude
};

// A prepared GLWE switch key (tfhe_prepare_glwe_switch_key): one packing slice of dimension k -- (k+1) l_ks key rows, the
// last l_ks zero spectra -- on the device of the context that prepared it, for that context's backend, ring and KS levels.
struct tfhe_glwe_switch_key {
  const tfhe_context* owner = nullptr;  // compared, never dereferenced
  int device = 0;
  int field = 0;
  u32 log_n = 0, k = 0, levels = 0;
  DeviceBuffer d_key;  // [(k+1) l_ks][k+1][parts][N] 8-byte words (spectrum_slot order, x 1/N)
};

// A prepared multi-bit bootstrapping key (tfhe_prepare_multibit_key): the raw u32 GGSWs [ceil(n / g)][2^g - 1][(k+1) l][k+1][N]
// on the device of the context that prepared it -- the bundle launch reads them word by word (multibit.h), nothing is
// transformed ahead of a call.
struct tfhe_multibit_key {
  const tfhe_context* owner = nullptr;  // compared, never dereferenced
  int device = 0;
  u32 g = 0, groups = 0;
  DeviceBuffer d_key;
};

namespace tfhe {
namespace host {

inline int fail(tfhe_context* ctx, int status, const std::string& msg) {
  if (ctx) ctx->last_error = msg;
  return status;
}

inline int hip_fail(tfhe_context* ctx, hipError_t e, const char* what) {
  return fail(ctx, TFHE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// pool.cpp: allocate dst's key buffers like src's and copy the PREPARED bootstrapping key and the key-switching
// key (raw and, where the matrix path is admitted, prepared) device to device (peer copy over xGMI, or a plain device copy when both contexts sit on one GPU) on dst's
// stream; dst must have been created with the same parameters and backend (capi.cpp)
int adopt_prepared_key(tfhe_context* dst, const tfhe_context* src);

// Sizes, each spelled out once.  32-bit words unless the name says otherwise.
inline size_t glwe_words(const tfhe_context* ctx) { return (size_t)(ctx->params.glwe_dimension + 1) * ctx->N; }
inline size_t lwe_words(const tfhe_context* ctx) { return (size_t)ctx->params.lwe_dimension + 1; }  // an LWE at n
inline size_t big_lwe_words(const tfhe_context* ctx) { return (size_t)ctx->big_n + 1; }             // an LWE at k*N
// words of one ciphertext at the bootstrap boundary (n+1, or k*N+1 in KS-first order)
inline size_t io_words(const tfhe_context* ctx) { return ctx->ks_first ? big_lwe_words(ctx) : lwe_words(ctx); }
inline size_t ggsw_words(const tfhe_context* ctx) { return (size_t)ctx->R * glwe_words(ctx); }  // a raw GGSW
inline size_t prepared_ggsw_words(const tfhe_context* ctx) { return ggsw_words(ctx) * ctx->parts; }  // 8-byte words
inline size_t ksk_words(const tfhe_context* ctx) { return (size_t)ctx->big_n * ctx->ks.levels * lwe_words(ctx); }
// the matrix-core key switch serves this context's key-switch decomposer (ks_matrix.h::ksm_admitted)
inline bool ks_matrix_admitted(const tfhe_context* ctx) { return ksm_admitted(ctx->ks.log_base, ctx->ks.levels, ctx->big_n); }
inline size_t ksk_matrix_bytes(const tfhe_context* ctx) {
  return launch::ksk_matrix_bytes(ctx->ks, ctx->big_n, ctx->params.lwe_dimension);
}
// the raw packing key from an LWE key of `from_dimension` bits: one GLWE row per (key bit, KS level)
inline size_t packing_key_words(const tfhe_context* ctx, size_t from_dimension) {
  return from_dimension * ctx->ks.levels * glwe_words(ctx);
}
// the raw GLWE switch key: one GLWE row per (polynomial of the source key, KS level)
inline size_t glwe_switch_key_words(const tfhe_context* ctx) {
  return (size_t)ctx->params.glwe_dimension * ctx->ks.levels * glwe_words(ctx);
}
// the multi-bit key for g bits per group: 2^g - 1 raw GGSWs per group of key bits
inline size_t multibit_groups(const tfhe_context* ctx, unsigned g) { return ((size_t)ctx->params.lwe_dimension + g - 1) / g; }
inline size_t multibit_key_ggsws(const tfhe_context* ctx, unsigned g) { return multibit_groups(ctx, g) * (((size_t)1 << g) - 1); }
// the bundles of `batch` samples: one prepared GGSW per (sample, group)
inline size_t multibit_bundle_bytes(const tfhe_context* ctx, size_t batch, unsigned g) {
  return batch * multibit_groups(ctx, g) * prepared_ggsw_words(ctx) * sizeof(u64);
}
inline size_t prepared_bsk_bytes(const tfhe_context* ctx, size_t ggsws) {
  return ggsws * prepared_ggsw_words(ctx) * sizeof(u64);
}

}  // namespace host
}  // namespace tfhe

// return from the calling function unless a HIP call / a call that returns a tfhe status succeeded
#define HIP_TRY(ctx, expr)                                              \
  do {                                                                  \
    hipError_t _e = (expr);                                             \
    if (_e != hipSuccess) return tfhe::host::hip_fail((ctx), _e, #expr); \
  } while (0)

#define TFHE_TRY(expr)          \
  do {                          \
    int _st = (expr);           \
    if (_st != TFHE_OK) return _st; \
  } while (0)

// the one place that allocates and frees device memory (DeviceBuffer above states the rule it keeps)
inline int DeviceBuffer::reallocate(tfhe_context* ctx, size_t bytes) {
  void* old = ptr_;
  ptr_ = nullptr;
  bytes_ = 0;
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (old) {  // freed whatever the stream said: nothing else holds it
    const hipError_t freed = hipFree(old);
    if (e == hipSuccess) e = freed;
  }
  if (e == hipSuccess && bytes && (e = hipMalloc(&ptr_, bytes)) != hipSuccess) ptr_ = nullptr;
  if (e != hipSuccess) return tfhe::host::hip_fail(ctx, e, "DeviceBuffer (hipStreamSynchronize / hipFree / hipMalloc)");
  bytes_ = bytes;
  return TFHE_OK;
}
