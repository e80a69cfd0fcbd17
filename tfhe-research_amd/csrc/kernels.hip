// kernels.hip -- gfx950 (CDNA4 / MI355X) kernels of the TFHE bootstrapping hot path.
//
// Execution shape: one workgroup = one TEAM of K+1 groups of G wavefronts = one LWE sample; group c
// owns GLWE polynomial c and output column c (pbs_wave.h).  G = 1 up to N = 1024 (transforms are
// wave-local, no barrier inside), G = 4 at N = 2048 (one cross-wave transpose per transform).  The
// team meets at a workgroup barrier once or twice per gadget level (two or one LDS exchange
// buffers per group) to hand the digit spectra around.
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "glwe_conv.h"
#include "glwe_switch.h"
#include "launch.h"
#include "lwe_dense.h"
#include "lwe_extract.h"
#include "multi_value.h"
#include "passes.h"
#include "radix.h"
#include "seeded.h"

namespace tfhe {
namespace {

using passes::kMaxGrid;

// waves per polynomial: one, except N = 2048, where four waves hold 8 elements per array each.
// (With two waves -- 16 elements, 256 VGPRs -- a k = 2 team is 6 waves on a CU that then has room
// for 8: SIMDs end up with 2, 2, 1, 1 waves and the team runs at the pace of the shared ones.  Four
// waves per polynomial fit 170 VGPRs, so the 12-wave team sits 3, 3, 3, 3.)
// (N = 1024 over two waves was measured too: 97.9 ms against 64.0 ms per cfg2 batch -- a fourth
// register pass and cross-wave barriers cost more than the third wave per SIMD gives; the complex transform at
// N = 1024 over two waves, 4 elements per lane with registers for two samples per team, lost as well:
// profiles/r03_kernel_ab.txt.)
// The complex transform has N/2 elements of 16 bytes: four waves per polynomial at N = 2048 hold 4 of them per lane
// and array (two waves, 8 per lane -- the register footprint of one wave at N = 1024 -- make one 6-wave team per CU:
// see field_shape_ok).
constexpr int kGroupN2048 = 4;
template <class F, int LOGN>
struct GroupOf {
  static constexpr int value = (LOGN >= 11) ? kGroupN2048 : 1;
};

// Shapes a transform policy is instantiated for.  The complex transform (field_fft.h) holds two
// coefficients per element, so its N/2-point transform has 8 elements per lane at N = 1024 with one wave
// per polynomial and 4 at N = 512 (four register passes of two bits); N = 2048 is bit-exact both over two waves per
// polynomial (8 elements per lane, one 6-wave team per CU: 137 ms per 1024 cfg5 bootstraps) and over four (4 elements
// per lane, five register passes, 12 waves: 79.2 ms) but does not beat the 42-bit field's 77.2 ms -- a 12-wave team
// is bound by its barriers, not its arithmetic (profiles/r02_kernel_ab.txt).  What is instantiated at N = 2048 is
// the complex transform over four waves per polynomial (4 elements per lane, five register passes) with TWO samples
// per team -- 57.4 ms per 1024 cfg5 bootstraps against 77.5 ms for the 42-bit field and 80.1 ms with one sample per
// team (profiles/r03_kernel_ab.txt).
template <class F, int LOGN>
constexpr bool field_shape_ok() {
  return F::kLogShrink == 0 || (LOGN >= 9 && LOGN <= 11);
}

// bytes of the twiddle table of a field at ring degree 2^LOGN
template <class F, int LOGN>
constexpr size_t twiddle_bytes() {
  return (size_t)ntt_twiddle_words(1 << (LOGN - F::kLogShrink)) * sizeof(typename F::elem);
}
// entries of it the working copy in LDS needs: the fused-stage constants behind psi_rev[N) are read through the
// uniform pointer only, and fields without fused stages do not have them at all -- 288 bytes that decide whether
// a fourth team fits a CU at N = 512, k = 2 and whether two samples fit the one team of N = 2048
template <class F, int LOGN>
constexpr int staged_twiddle_words() {
  return F::kFuseFirstTwo ? ntt_twiddle_words(1 << (LOGN - F::kLogShrink)) : (1 << (LOGN - F::kLogShrink));
}

template <class Elem, int G, int EXB = 1>
struct DeviceWave {
  unsigned char* team_base_;  // LDS of group 0 of this team (its exchange buffer in use)
  Elem* scratch_;             // my group's exchange / transpose buffer in use
  u32* acc_;
  const Elem* tw_;
  const Elem* twg_;           // the natural-order table in global memory (kernel argument: uniform)
  int group_;                 // polynomial / output column of my group
  unsigned group_stride_;     // bytes of LDS per group
  unsigned buffer_bytes_;     // bytes of one exchange buffer (EXB of them per group, back to back)
  unsigned acc_words_;        // u32 words of one accumulator polynomial (one per sample of the team, back to back)
  // number of exchange buffers per group and a copy of this context that works in buffer i
  // (pbs_wave.h::external_product_team); buffer 0 is the one selected at construction
  __device__ __forceinline__ int exchange_buffers() const { return EXB; }
  __device__ __forceinline__ DeviceWave with_exchange_buffer(int i) const {
    DeviceWave w = *this;
    if (EXB > 1) {
      w.team_base_ += (size_t)i * buffer_bytes_;
      w.scratch_ = reinterpret_cast<Elem*>(reinterpret_cast<unsigned char*>(scratch_) + (size_t)i * buffer_bytes_);
    }
    return w;
  }
  // thread index inside my polynomial's group of G waves
  __device__ __forceinline__ int tid() const { return (int)(threadIdx.x & (64u * G - 1u)); }
  __device__ __forceinline__ int group() const { return group_; }
  // Orders LDS stores of my polynomial's group before its later LDS loads.  G == 1: all 64 lanes run
  // in lockstep and the LDS pipeline is in-order per wave, so only the compiler has to be fenced.
  // G > 1: the group spans waves, so this is the workgroup barrier (every wave of the workgroup runs
  // the same transforms, hence the same number of barriers).
  __device__ __forceinline__ void poly_sync() const {
    if (G == 1) {
      wave_sync();
    } else {
      __syncthreads();
    }
  }
  // Orders the LDS stores of this wave's lanes before their later LDS loads (wave-local exchanges)
  __device__ __forceinline__ void wave_sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // workgroup barrier: the team of K+1 groups that shares one sample IS the workgroup
  // (timing experiments with the barriers compiled out: cfg2 -1 %, cfg3 20 % SLOWER -- there they cost
  // next to nothing and keep the team's key accesses together; cfg5, one 12-wave team per CU and 13
  // workgroup barriers per product: 78.6 -> 67.2 ms, i.e. 14.5 % of that kernel is barrier wait.  A
  // barrier scoped to the 4 waves of one polynomial group (LDS arrival counter + bounded spin) for the
  // 8 barriers that only order a group's cross-wave transposes was built and measured: bit-exact, same
  // time (78.88 vs 78.95 ms) -- the wait is the drift between waves that share SIMDs three at a time,
  // whatever the scope.  profiles/r02_kernel_ab.txt)
  // (TFHE_PROBE_NO_TEAM_SYNC: dev_switches.h -- a WRONG-BITS timing probe, TFHE_DEV_BUILD only)
  __device__ __forceinline__ void team_sync() const {
    if (!TFHE_PROBE_NO_TEAM_SYNC) __syncthreads();
  }
  __device__ __forceinline__ Elem* scratch() const { return scratch_; }
  __device__ __forceinline__ const Elem* scratch_of(int s) const {
    return reinterpret_cast<const Elem*>(team_base_ + (size_t)s * group_stride_);
  }
  __device__ __forceinline__ u32* acc(int s = 0) const { return acc_ + (size_t)s * acc_words_; }
  __device__ __forceinline__ const Elem* twiddles() const { return tw_; }
  __device__ __forceinline__ const Elem* twiddles_uniform() const { return twg_; }
  __device__ __forceinline__ u32 uniform(u32 v) const { return __builtin_amdgcn_readfirstlane(v); }
  // *p += v on an LDS word this lane owns: one ds_add_u32 (no return value) instead of a read, an add and a write
  __device__ __forceinline__ void lds_add(u32* p, u32 v) const {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // compiler-only barrier: memory operations are not moved across it
  __device__ __forceinline__ void compiler_fence() const { asm volatile("" ::: "memory"); }
};

// One workgroup = one team = K+1 polynomial groups of G waves = one LWE sample.
// LDS (dynamic, 16-B aligned base, no static LDS): [ twiddles (N+2) x 8 B ][ group c: EXB transpose/
// exchange buffers of N x 8 B | accumulator polynomial N x 4 B ] for c = 0..K
// Exchange buffers per group: two (one team barrier per gadget level instead of two) at N = 2048,
// where one 12-wave team per CU leaves LDS to spare and the barriers of a 768-thread workgroup are
// dear (+5 % at cfg5).  One at N = 1024 (4 teams per CU would need 192 KiB with two) and at N = 512
// (two fit, 139 KiB, but measured no gain at cfg3: 114.6 vs 116.1 ms per 4096 gates).
template <int LOGN>
struct ExchangeBuffersOf {
  static constexpr int value = (LOGN >= 11) ? 2 : 1;
};

// (Two and four teams per workgroup -- one barrier sequence, one twiddle table, the second wave that asks for
// a key tile finding it in the CU's vector L1 -- were measured for the complex transform, whose kernel draws
// 13 TB/s of key from L2: 41.5 and 46.4 ms against 37.1 ms with one team per workgroup.  Teams that are free
// to drift fill each other's stalls; coupling them costs more than the L1 hits give.)
// Samples per team in the blind rotation (pbs_wave.h::external_product_team_multi): two where the registers allow it
// (the complex transform with 4 elements per lane) AND the kernel waits on its key stream or its barriers -- the
// twelve-wave team of N = 2048 and the many digit rows of N = 512, k = 2.  Measured per shape, profiles/r03_kernel_ab.txt.
template <class F, int LOGN, int K>
struct SamplesPerTeam {
  static constexpr int value = (F::kLogShrink && (LOGN == 11 || (LOGN == 9 && K == 2))) ? 2 : 1;
};

template <class F, int LOGN, int K, int NS_ = SamplesPerTeam<F, LOGN, K>::value>
struct TeamCfg {
  static constexpr int N = 1 << LOGN;
  static constexpr int G = GroupOf<F, LOGN>::value;
  static constexpr int S = NS_;  // samples per team: each has an exchange buffer and an accumulator per group
  static constexpr int EXB = ExchangeBuffersOf<LOGN>::value > S ? ExchangeBuffersOf<LOGN>::value : S;
  static constexpr int kWaves = (K + 1) * G;
  static constexpr int kThreads = kWaves * 64;
  static constexpr unsigned kGroupLds = (unsigned)N * 8u * EXB + (unsigned)N * 4u * S;
  // the working copy of the table: (N + 18) 8-byte elements, or N/2 16-byte ones
  static constexpr size_t kTwBytes = (size_t)staged_twiddle_words<F, LOGN>() * sizeof(typename F::elem);  // multiple of 16
  static constexpr size_t kLds = kTwBytes + (size_t)(K + 1) * kGroupLds;
  // waves per SIMD the kernels' register budget is set for: three in the shapes with 8 ring coefficients per lane and
  // array, two elsewhere
  static constexpr int kMinWaves = (NttShape<LOGN, G>::kE == 8) ? 3 : 2;
};

template <class F, int LOGN, int K, int NS = SamplesPerTeam<F, LOGN, K>::value>
__device__ __forceinline__ DeviceWave<typename F::elem, GroupOf<F, LOGN>::value, TeamCfg<F, LOGN, K, NS>::EXB>
make_wave(unsigned char* smem, const typename F::elem* tw_global) {
  typedef typename F::elem elem;
  using C = TeamCfg<F, LOGN, K, NS>;
  static_assert(C::kTwBytes % 16 == 0, "twiddle table");
  elem* tw = reinterpret_cast<elem*>(smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, C::G, elem, staged_twiddle_words<F, LOGN>()>(tw, tw_global, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  DeviceWave<elem, C::G, C::EXB> w;
  w.group_ = (int)(threadIdx.x / (64u * C::G));
  w.group_stride_ = C::kGroupLds;
  w.buffer_bytes_ = (unsigned)C::N * 8u;
  w.acc_words_ = (unsigned)C::N;
  w.team_base_ = smem + C::kTwBytes;
  unsigned char* base = w.team_base_ + (size_t)w.group_ * C::kGroupLds;
  w.tw_ = tw;
  w.twg_ = tw_global;
  w.scratch_ = reinterpret_cast<elem*>(base);
  w.acc_ = reinterpret_cast<u32*>(base + (size_t)C::N * 8 * C::EXB);
  return w;
}

extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];

// ------------------------------------------------------------------------------ bsk_prepare
// one polynomial per group of G waves; kPolysPerBlock groups per workgroup
template <class F, int LOGN>
__global__ void __launch_bounds__(256) bsk_prepare_kernel(const typename F::elem* __restrict__ tw,
                                                         const u32* __restrict__ polys,
                                                         size_t poly_count,
                                                         typename F::elem* __restrict__ spectra,
                                                         typename F::elem n_inv, int layout_e) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr int G = GroupOf<F, LOGN>::value;
  elem* twl = reinterpret_cast<elem*>(g_smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, G>(twl, tw, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  const int group = (int)(threadIdx.x / (64u * G));
  const int groups = (int)(blockDim.x / (64u * G));
  // For G > 1 the transform contains workgroup barriers, so every group of the block has to run it:
  // a group past the end of the list redoes the last polynomial (same values to the same addresses).
  size_t poly = (size_t)blockIdx.x * groups + group;
  if (poly >= poly_count) {
    if (G == 1) return;
    poly = poly_count - 1;
  }
  DeviceWave<elem, G> w;
  w.group_ = 0;
  w.group_stride_ = 0;
  w.buffer_bytes_ = 0;
  w.acc_words_ = 0;
  w.team_base_ = nullptr;
  w.tw_ = twl;
  w.twg_ = tw;
  w.scratch_ = reinterpret_cast<elem*>(g_smem + twiddle_bytes<F, LOGN>() + (size_t)group * N * 8);
  w.acc_ = nullptr;
  // the key's layout (pbs_wave.h::key_layout_e): the pair kernel's at N = 512, k = 1 in the complex transform
  if constexpr (key_layout_e<F, LOGN, 1>() != 0) {
    if (layout_e == key_layout_e<F, LOGN, 1>()) {
      bsk_prepare_wave<F, LOGN, G, key_layout_e<F, LOGN, 1>()>(w, polys + poly * N, spectra + poly * (N >> F::kLogShrink) * F::kParts, n_inv);
      return;
    }
  }
  bsk_prepare_wave<F, LOGN, G>(w, polys + poly * N, spectra + poly * (N >> F::kLogShrink) * F::kParts, n_inv);
}

// ------------------------------------------------------------------------------ blind rotation
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K>::kThreads), (TeamCfg<F, LOGN, K>::kMinWaves))
blind_rotate_kernel(PbsParams P, const typename F::elem* __restrict__ tw,
                    const u32* __restrict__ lwe_in, size_t batch, const u32* __restrict__ tv,
                    size_t tv_stride, const typename F::elem* __restrict__ bsk,
                    u32* glwe_out /* may be glwe_state (the caller's output parks the accumulators): no restrict */,
                    u32* __restrict__ lwe_extracted,
                    u32 i_begin, u32 i_end, u32* glwe_state /* [batch][K+1][N]: accumulators between segments */) {
  using C = TeamCfg<F, LOGN, K>;
  constexpr int N = C::N;
  constexpr int G = C::G;
  constexpr int NS = C::S;
  constexpr int E = NttShape<LOGN, G>::kE;
  constexpr int T = NttShape<LOGN, G>::kThreads;
  auto w = make_wave<F, LOGN, K>(g_smem, tw);
  // grid = ceil(batch / NS) teams of NS samples; every wave runs every barrier.  An odd batch leaves the last team
  // one sample short: it redoes the last sample in the free slot (same inputs, no output)
  size_t sample[NS];
  const u32* lwes[NS];
  const u32* tvs[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const size_t idx = (size_t)blockIdx.x * NS + s;
    sample[s] = idx < batch ? idx : batch - 1;
    lwes[s] = lwe_in + sample[s] * (P.n + 1);
    tvs[s] = tv + sample[s] * tv_stride;
  }

  const u32* resume[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) resume[s] = i_begin > 0 ? glwe_state + sample[s] * (size_t)(K + 1) * N : nullptr;  // (null state: one launch)
  blind_rotate_team_multi<F, LOGN, K, G, NS>(w, P, lwes, tvs, bsk, i_begin, i_end, resume);

  const int tid = w.tid();
  if (i_end < P.n) {  // not the last segment: park the accumulators
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if ((size_t)blockIdx.x * NS + s >= batch) break;
      u32* dst = glwe_state + (sample[s] * (size_t)(K + 1) + w.group()) * N;
#pragma unroll
      for (int r = 0; r < E; ++r) dst[r * T + tid] = w.acc(s)[r * T + tid];
    }
    return;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if ((size_t)blockIdx.x * NS + s >= batch) break;  // the duplicate of an odd batch's last sample
    if (glwe_out) {
      u32* dst = glwe_out + (sample[s] * (size_t)(K + 1) + w.group()) * N;
#pragma unroll
      for (int r = 0; r < E; ++r) dst[r * T + tid] = w.acc(s)[r * T + tid];
    }
    if (lwe_extracted) sample_extract_team<LOGN, K, G>(w, lwe_extracted + sample[s] * ((size_t)K * N + 1), s);
  }
}

// ------------------------------------------------------------------------------ blind rotation, pair kernel
// ONE wavefront per sample at k = 1, N = 512 in the complex transform (pbs_wave.h::blind_rotate_pair): polynomial c in lanes
// 32 c .. 32 c + 31, 8 elements per lane, no workgroup barrier.  The shape's throughput kernel (the launch plan -- key
// slices, two streams -- is the team kernel's: launch_blind_rotate); same arguments as blind_rotate_kernel.
// LDS: [ twiddles ][ half 0: buffer N x 4 B... | half 1 ] = 4 KiB + 2 x 4 KiB buffers + 2 x 2 KiB accumulator polynomials.
template <class F, int LOGN, int K>
constexpr bool pair_shape() {
  return F::kLogShrink == 1 && F::kParts == 2 && LOGN == 9 && K == 1;
}
template <class Elem>
struct PairWave {
  unsigned char* buffers_;  // half 0's transpose / exchange buffer; half 1's follows
  u32* accs_;               // accumulator polynomial 0; polynomial 1 follows
  const Elem* tw_;
  const Elem* twg_;
  unsigned buffer_bytes_, acc_words_;
  __device__ __forceinline__ int tid() const { return (int)(threadIdx.x & 31u); }
  __device__ __forceinline__ int group() const { return (int)((threadIdx.x >> 5) & 1u); }
  __device__ __forceinline__ void wave_sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ void poly_sync() const { wave_sync(); }
  __device__ __forceinline__ void team_sync() const { wave_sync(); }  // the team is this wave
  __device__ __forceinline__ Elem* scratch() const { return reinterpret_cast<Elem*>(buffers_ + (size_t)group() * buffer_bytes_); }
  __device__ __forceinline__ const Elem* scratch_of(int half) const { return reinterpret_cast<const Elem*>(buffers_ + (size_t)half * buffer_bytes_); }
  __device__ __forceinline__ u32* acc(int = 0) const { return accs_ + (size_t)group() * acc_words_; }
  __device__ __forceinline__ const Elem* twiddles() const { return tw_; }
  __device__ __forceinline__ const Elem* twiddles_uniform() const { return twg_; }
  __device__ __forceinline__ u32 uniform(u32 v) const { return __builtin_amdgcn_readfirstlane(v); }
  __device__ __forceinline__ void lds_add(u32* p, u32 v) const {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void compiler_fence() const { asm volatile("" ::: "memory"); }
};

template <class F, int LOGN>
struct PairCfg {
  static constexpr int N = 1 << LOGN;
  static constexpr int kThreads = 64;
  static constexpr size_t kTwBytes = (size_t)staged_twiddle_words<F, LOGN>() * sizeof(typename F::elem);
  static constexpr unsigned kBufferBytes = (unsigned)N * 8u;
  static constexpr size_t kLds = kTwBytes + 2 * (size_t)kBufferBytes + 2 * (size_t)N * 4;
};

constexpr int kPairMinWaves = 2;  // 2 waves per SIMD = 8 samples per CU, at the N = 1024 kernel's register footprint
template <class F, int LOGN>
__global__ void __launch_bounds__(64, kPairMinWaves)
blind_rotate_pair_kernel(PbsParams P, const typename F::elem* __restrict__ tw, const u32* __restrict__ lwe_in, size_t batch,
                         const u32* __restrict__ tv, size_t tv_stride, const typename F::elem* __restrict__ bsk,
                         u32* glwe_out, u32* __restrict__ lwe_extracted, u32 i_begin, u32 i_end, u32* glwe_state) {
  typedef typename F::elem elem;
  using C = PairCfg<F, LOGN>;
  constexpr int N = C::N;
  constexpr int T = 32;
  constexpr int EC = N / T;
  constexpr int K = 1;
  elem* twl = reinterpret_cast<elem*>(g_smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, 0, elem, staged_twiddle_words<F, LOGN>()>(twl, tw, (int)threadIdx.x, 64);
  __syncthreads();
  PairWave<elem> w;
  w.buffers_ = g_smem + C::kTwBytes;
  w.buffer_bytes_ = C::kBufferBytes;
  w.accs_ = reinterpret_cast<u32*>(w.buffers_ + 2 * (size_t)C::kBufferBytes);
  w.acc_words_ = (unsigned)N;
  w.tw_ = twl;
  w.twg_ = tw;
  const size_t sample = blockIdx.x;  // grid = batch
  (void)batch;
  const u32* resume = i_begin > 0 ? glwe_state + sample * (size_t)(K + 1) * N : nullptr;
  blind_rotate_pair<F, LOGN>(w, P, lwe_in + sample * (P.n + 1), tv + sample * tv_stride, bsk, i_begin, i_end, resume);
  const int tid = w.tid(), me = w.group();
  const u32* acc = w.acc();
  if (i_end < P.n) {  // not the last segment: park the accumulators
    u32* dst = glwe_state + (sample * (size_t)(K + 1) + me) * N;
#pragma unroll
    for (int r = 0; r < EC; ++r) dst[r * T + tid] = acc[r * T + tid];
    return;
  }
  if (glwe_out) {
    u32* dst = glwe_out + (sample * (size_t)(K + 1) + me) * N;
#pragma unroll
    for (int r = 0; r < EC; ++r) dst[r * T + tid] = acc[r * T + tid];
  }
  if (lwe_extracted) {  // sample_extract at index 0 (bootstrapping.rs:122-156)
    u32* out = lwe_extracted + sample * ((size_t)K * N + 1);
    if (me < K) {
#pragma unroll
      for (int r = 0; r < EC; ++r) {
        const int x = r * T + tid;
        out[me * N + x] = (x == 0) ? acc[0] : (0u - acc[N - x]);
      }
    } else if (tid == 0) {
      out[K * N] = acc[0];
    }
  }
}

// The kernel that rotates a shape's large batches, with what the launcher needs to know about it
template <class F, int LOGN, int K>
struct RotateKernel {
  using C = TeamCfg<F, LOGN, K>;
  static constexpr int kThreads = C::kThreads;
  static constexpr size_t kLds = C::kLds;
  static constexpr int kSamples = C::S;   // samples per workgroup
  static constexpr int kWaves = C::kWaves;
  static auto get() { return blind_rotate_kernel<F, LOGN, K>; }
};
template <int LOGN, int K>
struct RotateKernelPair {
  using C = PairCfg<FftField, LOGN>;
  static constexpr int kThreads = C::kThreads;
  static constexpr size_t kLds = C::kLds;
  static constexpr int kSamples = 1;
  static constexpr int kWaves = 1;
  static auto get() { return blind_rotate_pair_kernel<FftField, LOGN>; }
};
template <class F, int LOGN, int K>
using PairOrTeamKernel = typename std::conditional<pair_shape<F, LOGN, K>(), RotateKernelPair<LOGN, K>, RotateKernel<F, LOGN, K>>::type;

// ------------------------------------------------------------------------------ blind rotation, wide team
// The latency shape (pbs_wave.h::blind_rotate_team_wide): 2 (K+1) waves per sample -- wave (c, q) transforms half of
// polynomial c's digit levels, accumulates key part q of column c over all rows and inverse-transforms that one
// accumulator.  The complex transform up to N = 1024.  Picked by the launcher for batches that leave most CUs idle.
// LDS: [ twiddles ][ (K+1) l row buffers of N x 8 B ][ 2 (K+1) transpose buffers, one per wave ][ K+1 accumulator polynomials of N x 4 B ]
template <class Elem>
struct WideWave {
  unsigned char* rows_;  // row buffer 0
  Elem* scratch_;        // my own transpose buffer
  u32* acc_;             // my polynomial's accumulator
  const Elem* tw_;
  const Elem* twg_;
  unsigned row_bytes_;
  int wave_;             // 2 c + q
  __device__ __forceinline__ int tid() const { return (int)(threadIdx.x & 63u); }
  __device__ __forceinline__ int group() const { return wave_ >> 1; }
  __device__ __forceinline__ int half() const { return wave_ & 1; }
  __device__ __forceinline__ Elem* row_buffer(int r) const { return reinterpret_cast<Elem*>(rows_ + (size_t)r * row_bytes_); }
  __device__ __forceinline__ void wave_sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ void poly_sync() const { wave_sync(); }  // one wave per transform
  __device__ __forceinline__ void team_sync() const { __syncthreads(); }
  __device__ __forceinline__ Elem* scratch() const { return scratch_; }
  __device__ __forceinline__ u32* acc(int = 0) const { return acc_; }
  __device__ __forceinline__ const Elem* twiddles() const { return tw_; }
  __device__ __forceinline__ const Elem* twiddles_uniform() const { return twg_; }
  __device__ __forceinline__ u32 uniform(u32 v) const { return __builtin_amdgcn_readfirstlane(v); }
  __device__ __forceinline__ void lds_add(u32* p, u32 v) const {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void compiler_fence() const { asm volatile("" ::: "memory"); }
};

template <class F, int LOGN, int K>
struct WideCfg {
  static constexpr int N = 1 << LOGN;
  static constexpr int kWaves = 2 * (K + 1);
  static constexpr int kThreads = kWaves * 64;
  static constexpr size_t kTwBytes = (size_t)staged_twiddle_words<F, LOGN>() * sizeof(typename F::elem);
  static constexpr unsigned kRowBytes = (unsigned)N * 8u;
  static __host__ __device__ size_t row_buffers(u32 levels) { return (size_t)(K + 1) * levels + kWaves; }  // rows, then one per wave
  static __host__ __device__ size_t lds(u32 levels) { return kTwBytes + row_buffers(levels) * kRowBytes + (size_t)(K + 1) * N * 4; }
};

// Key ring of the wide team (pbs_wave.h::WideKeyRing): rows of a wave's key tiles held in registers ahead of time.
// LEVELS > 0 instantiates the kernel for that level count (the ring's slots are compile-time); LEVELS = 0 is the generic
// kernel (run-time level count, key chunks one ahead).  Register budget: a k = 1 team is four waves, one per SIMD, and
// one team per CU is all its LDS allows -- a wave may use the SIMD's whole file (512 registers: the allocator takes
// AGPRs beyond 256): 224 for the ring; a k = 2 team's six waves put two on two of the SIMDs: 256 each, 112 for the ring.
constexpr int kWideMinWaves = 2;  // waves per SIMD of the generic kernel and of a k = 2 team (its six waves double up on two SIMDs)
template <class F, int LOGN, int K, int LEVELS>
__global__ void __launch_bounds__((WideCfg<F, LOGN, K>::kThreads), (K == 1 && LEVELS > 0 ? 1 : kWideMinWaves))
blind_rotate_wide_kernel(PbsParams P, const typename F::elem* __restrict__ tw, const u32* __restrict__ lwe_in, size_t batch,
                         const u32* __restrict__ tv, size_t tv_stride, const typename F::elem* __restrict__ bsk,
                         u32* glwe_out, u32* __restrict__ lwe_extracted, u32 i_begin, u32 i_end, u32* glwe_state) {
  typedef typename F::elem elem;
  using C = WideCfg<F, LOGN, K>;
  constexpr int N = C::N;
  constexpr int EC = N / 64;
  elem* twl = reinterpret_cast<elem*>(g_smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, 1, elem, staged_twiddle_words<F, LOGN>()>(twl, tw, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  WideWave<elem> w;
  w.wave_ = (int)(threadIdx.x >> 6);
  w.rows_ = g_smem + C::kTwBytes;
  w.row_bytes_ = C::kRowBytes;
  w.scratch_ = reinterpret_cast<elem*>(w.rows_ + ((size_t)(K + 1) * P.levels + w.wave_) * C::kRowBytes);
  w.acc_ = reinterpret_cast<u32*>(w.rows_ + C::row_buffers(P.levels) * C::kRowBytes) + (size_t)w.group() * N;
  w.tw_ = twl;
  w.twg_ = tw;
  const size_t sample = blockIdx.x;  // grid = batch
  const u32* resume = i_begin > 0 ? glwe_state + sample * (size_t)(K + 1) * N : nullptr;
  blind_rotate_team_wide<F, LOGN, K, LEVELS, wide_ring_rows<LOGN, K, LEVELS>()>(w, P, lwe_in + sample * (P.n + 1), tv + sample * tv_stride, bsk,
                                                                               i_begin, i_end, resume);
  (void)batch;
  // each half stores the words it loaded: registers [q EC/2, (q + 1) EC/2) of polynomial c
  const int tid = w.tid(), me = w.group(), q = w.half();
  const u32* acc = w.acc();
  if (i_end < P.n) {  // not the last segment: park the accumulators
    u32* dst = glwe_state + (sample * (size_t)(K + 1) + me) * N;
#pragma unroll
    for (int r = 0; r < EC / 2; ++r) dst[(r + q * (EC / 2)) * 64 + tid] = acc[(r + q * (EC / 2)) * 64 + tid];
    return;
  }
  if (glwe_out) {
    u32* dst = glwe_out + (sample * (size_t)(K + 1) + me) * N;
#pragma unroll
    for (int r = 0; r < EC / 2; ++r) dst[(r + q * (EC / 2)) * 64 + tid] = acc[(r + q * (EC / 2)) * 64 + tid];
  }
  if (lwe_extracted) {  // sample_extract at index 0 (bootstrapping.rs:122-156), the words split between the halves
    u32* out = lwe_extracted + sample * ((size_t)K * N + 1);
    if (me < K) {
#pragma unroll
      for (int r = 0; r < EC / 2; ++r) {
        const int x = (r + q * (EC / 2)) * 64 + tid;
        out[me * N + x] = (x == 0) ? acc[0] : (0u - acc[N - x]);
      }
    } else if (q == 0 && tid == 0) {
      out[K * N] = acc[0];
    }
  }
}

// ------------------------------------------------------------------------------ multi-bit blind rotation
// multibit.h states the two steps.  The bundle launch is bsk_prepare_kernel's shape -- one polynomial per wave, four per
// workgroup -- over (every polynomial of every group's bundle, the batch): at cfg2 with g = 3 that is 630 workgroups per
// sample, the launch that fills the chip at batch 1.  The rotate launch is blind_rotate_wide_kernel's: one wide team per
// sample, its key the sample's own bundles.
template <class F, int LOGN, int GBITS>
__global__ void __launch_bounds__(256) multibit_bundle_kernel(const typename F::elem* __restrict__ tw, const u32* __restrict__ key,
                                                             const u32* __restrict__ lwe_in, u32 n, u32 groups, u32 ggsw_polys,
                                                             typename F::elem* __restrict__ bundles, typename F::elem n_inv, int layout_e) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  static_assert(GroupOf<F, LOGN>::value == 1, "one wave per polynomial: a wave past the end of the list may leave");
  elem* twl = reinterpret_cast<elem*>(g_smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, 1>(twl, tw, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  const int wave = (int)(threadIdx.x / 64u);
  const size_t polys = (size_t)groups * ggsw_polys;  // of one sample's bundles
  const size_t poly = (size_t)blockIdx.x * (blockDim.x / 64u) + wave;
  if (poly >= polys) return;
  const size_t sample = blockIdx.y;
  DeviceWave<elem, 1> w;
  w.group_ = 0;
  w.group_stride_ = 0;
  w.buffer_bytes_ = 0;
  w.acc_words_ = 0;
  w.team_base_ = nullptr;
  w.tw_ = twl;
  w.twg_ = tw;
  w.scratch_ = reinterpret_cast<elem*>(g_smem + twiddle_bytes<F, LOGN>() + (size_t)wave * N * 8);
  w.acc_ = nullptr;
  const u32 group = w.uniform((u32)(poly / ggsw_polys)), rc = w.uniform((u32)(poly % ggsw_polys));
  const u32* lwe = lwe_in + sample * ((size_t)n + 1);
  elem* spec = bundles + (sample * polys + poly) * (N >> F::kLogShrink) * F::kParts;
  const size_t ggsw_words = (size_t)ggsw_polys * N;
  if constexpr (key_layout_e<F, LOGN, 1>() != 0) {
    if (layout_e == key_layout_e<F, LOGN, 1>()) {
      multibit_bundle_wave<F, LOGN, 1, GBITS, key_layout_e<F, LOGN, 1>()>(w, key, ggsw_words, lwe, n, group, rc, spec, n_inv);
      return;
    }
  }
  multibit_bundle_wave<F, LOGN, 1, GBITS, 0>(w, key, ggsw_words, lwe, n, group, rc, spec, n_inv);
}

// LDS and registers: blind_rotate_wide_kernel's (the key ring and its budget are explained there)
template <class F, int LOGN, int K, int LEVELS>
__global__ void __launch_bounds__((WideCfg<F, LOGN, K>::kThreads), (K == 1 && LEVELS > 0 ? 1 : kWideMinWaves))
multibit_rotate_wide_kernel(PbsParams P, const typename F::elem* __restrict__ tw, const u32* __restrict__ lwe_in,
                            const u32* __restrict__ tv, size_t tv_stride, const typename F::elem* __restrict__ bundles, u32 groups,
                            u32* glwe_out, u32* __restrict__ lwe_extracted) {
  typedef typename F::elem elem;
  using C = WideCfg<F, LOGN, K>;
  constexpr int N = C::N;
  elem* twl = reinterpret_cast<elem*>(g_smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, 1, elem, staged_twiddle_words<F, LOGN>()>(twl, tw, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  WideWave<elem> w;
  w.wave_ = (int)(threadIdx.x >> 6);
  w.rows_ = g_smem + C::kTwBytes;
  w.row_bytes_ = C::kRowBytes;
  w.scratch_ = reinterpret_cast<elem*>(w.rows_ + ((size_t)(K + 1) * P.levels + w.wave_) * C::kRowBytes);
  w.acc_ = reinterpret_cast<u32*>(w.rows_ + C::row_buffers(P.levels) * C::kRowBytes) + (size_t)w.group() * N;
  w.tw_ = twl;
  w.twg_ = tw;
  const size_t sample = blockIdx.x;  // grid = batch
  const size_t ggsw_elems = (size_t)(K + 1) * P.levels * (K + 1) * N;  // 2 parts x N/2 elements per polynomial
  multibit_rotate_team_wide<F, LOGN, K, LEVELS, wide_ring_rows<LOGN, K, LEVELS>()>(
      w, P, lwe_in + sample * (P.n + 1), tv + sample * tv_stride, bundles + sample * groups * ggsw_elems, groups,
      glwe_out ? glwe_out + sample * (size_t)(K + 1) * N : nullptr,
      lwe_extracted ? lwe_extracted + sample * ((size_t)K * N + 1) : nullptr);
}

// ------------------------------------------------------------------------------ block-binary blind rotation
// block_rotate.h states the step.  blind_rotate_kernel's shape with ONE sample per team whatever the shape's loop kernel
// takes: K+1 one-wave groups, the same LDS and register budget, segments [i_begin, i_end) that start on a block boundary
// and park their accumulators in glwe_state.  `block` is a kernel argument: one instantiation per (N, K).
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
block_rotate_kernel(PbsParams P, const typename F::elem* __restrict__ tw, const typename F::elem* __restrict__ roots,
                    const u32* __restrict__ lwe_in, const u32* __restrict__ tv, size_t tv_stride,
                    const typename F::elem* __restrict__ bsk, u32 block,
                    u32* glwe_out /* may be glwe_state: no restrict */, u32* __restrict__ lwe_extracted, u32 i_begin, u32 i_end,
                    u32* glwe_state /* [batch][K+1][N]: accumulators between segments */) {
  using C = TeamCfg<F, LOGN, K, 1>;
  constexpr int N = C::N;
  constexpr int E = NttShape<LOGN, 1>::kE;
  static_assert(C::G == 1 && C::EXB == 1, "one wave per polynomial, one exchange buffer");
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  const size_t sample = blockIdx.x;  // grid = batch
  block_rotate_team<F, LOGN, K>(w, P, lwe_in + sample * (P.n + 1), tv + sample * tv_stride, bsk, roots, block, i_begin, i_end,
                                i_begin > 0 ? glwe_state + sample * (size_t)(K + 1) * N : nullptr);
  const int tid = w.tid();
  if (i_end < P.n) {  // not the last segment: park the accumulators
    u32* dst = glwe_state + (sample * (size_t)(K + 1) + w.group()) * N;
#pragma unroll
    for (int r = 0; r < E; ++r) dst[r * 64 + tid] = w.acc()[r * 64 + tid];
    return;
  }
  if (glwe_out) {
    u32* dst = glwe_out + (sample * (size_t)(K + 1) + w.group()) * N;
#pragma unroll
    for (int r = 0; r < E; ++r) dst[r * 64 + tid] = w.acc()[r * 64 + tid];
  }
  if (lwe_extracted) sample_extract_team<LOGN, K, 1>(w, lwe_extracted + sample * ((size_t)K * N + 1));
}

// unrolled blind rotation (two key bits per step, pbs_wave.h::blind_rotate_bmmp_team); offered where a
// lane holds 8 elements per array and one wave owns a polynomial: N = 512
constexpr int kBmmpMinWaves = 3;
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), kBmmpMinWaves)
blind_rotate_bmmp_kernel(PbsParams P, const typename F::elem* __restrict__ tw,
                         const u32* __restrict__ lwe_in, size_t batch, const u32* __restrict__ tv,
                         size_t tv_stride, const typename F::elem* __restrict__ bsk,
                         u32* __restrict__ glwe_out, u32* __restrict__ lwe_extracted) {
  using C = TeamCfg<F, LOGN, K, 1>;
  constexpr int N = C::N;
  constexpr int G = C::G;
  constexpr int E = NttShape<LOGN, G>::kE;
  constexpr int T = NttShape<LOGN, G>::kThreads;
  static_assert(G == 1 && C::EXB == 1, "one wave per polynomial, one exchange buffer");
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  const size_t sample = blockIdx.x;
  blind_rotate_bmmp_team<F, LOGN, K, G>(w, P, lwe_in + sample * (P.n + 1), tv + sample * tv_stride, bsk);
  const int tid = w.tid();
  if (glwe_out) {
    u32* dst = glwe_out + (sample * (size_t)(K + 1) + w.group()) * N;
#pragma unroll
    for (int r = 0; r < E; ++r) dst[r * T + tid] = w.acc()[r * T + tid];
  }
  if (lwe_extracted) sample_extract_team<LOGN, K, G>(w, lwe_extracted + sample * ((size_t)K * N + 1));
}

// ------------------------------------------------------------------------------ external product
// Persistent grid: the launcher starts as many teams as are resident at once, so the twiddle table is
// staged into LDS once per team.  Short batches are handed out by stride (blockIdx.x, + gridDim.x, ...),
// long ones through a work queue.  Why both: a grid that exactly fills the chip with a FIXED share per
// team ends when its slowest CU does -- the same team code ran 7-12 % slower per product that way than
// under the dispatcher's dynamic placement of a larger grid -- so at 64 samples per team drawing tickets
// from a device counter is 5.7 % faster; with a handful of samples per team a queue only makes some
// teams take one more than the others (4 per team: +15 %, and +5 % even when only the tail is queued),
// so the launcher uses it from 16 samples per team (profiles/r02_external_product_experiments.txt).
// queue[0] hands out tickets; the launcher zeroes it on the stream right before the kernel (a memset node
// when the call is captured into a graph, so replays start from zero too).  Both forms of the reference call go through ONE
// instantiation of the team code: the plain product (ggsw.rs:132-161) and the CMUX form
// (ggsw.rs:164-178: ct1 -= ct0 is written back, the product is added to ct0); `cmux_ct0` is a kernel
// argument, so the selects below are wave-uniform branches.  (Measured and dropped: fetching the next
// sample's operand early -- by LDS-DMA or into registers behind the inverse transforms -- and starting
// the teams out of phase left the time per product unchanged within 2 %; with loads and stores compiled
// out the kernel is only 4 % faster.)
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
external_product_kernel(PbsParams P, const typename F::elem* __restrict__ tw,
                        const typename F::elem* __restrict__ ggsw, size_t ggsw_stride_words,
                        const u32* glwe_in, u32* ct1_inout, const u32* cmux_ct0, size_t batch,
                        u32* glwe_out, unsigned long long* queue /* null: by stride */) {
  using C = TeamCfg<F, LOGN, K, 1>;  // one product per team at a time (the samples have their own GGSWs in general)
  constexpr int N = C::N;
  constexpr int G = C::G;
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  const bool is_cmux = cmux_ct0 != nullptr;
  // the ticket of the team's current sample, published through LDS (behind the team's arrays)
  unsigned long long* ticket = reinterpret_cast<unsigned long long*>(g_smem + C::kLds);
  for (size_t turn = 0;; ++turn) {
    size_t sample;
    if (queue == nullptr) {
      sample = blockIdx.x + turn * gridDim.x;
    } else {
      if (threadIdx.x == 0) *ticket = atomicAdd(queue, 1ull);
      __syncthreads();  // every wave of the team sees the same ticket: the barriers below stay matched
      sample = (size_t)*ticket;
    }
    if (sample >= batch) break;
    const size_t poly = (sample * (size_t)(K + 1) + w.group()) * N;  // my polynomial / my output column
    const typename F::elem* g = ggsw + sample * ggsw_stride_words;
    const u32* in = is_cmux ? ct1_inout + poly : glwe_in + poly;
    const u32* c0 = cmux_ct0 + poly;
    u32* c1 = ct1_inout + poly;
    u32* dst = glwe_out + poly;
    // CMUX: each coefficient is read and written by the one lane that owns index j, so the in-place
    // update of ct1 (*glwe_ciphertext1 -= glwe_ciphertext0, ggsw.rs:171) is race free
    auto src = [&](int j) -> u32 {
      u32 d = __builtin_nontemporal_load(&in[j]);
      if (is_cmux) {
        d -= c0[j];
        c1[j] = d;
      }
      return d;
    };
    auto out = [&](int j, u32 v) { __builtin_nontemporal_store(is_cmux ? v + c0[j] : v, &dst[j]); };
    external_product_team<F, LOGN, K, G>(w, P, g, src, out);
    // (thread 0 overwrites the ticket only after the product's team barriers, which every wave passes
    // after it has read the ticket)
  }
}

// ------------------------------------------------------------------------------ packing key switch
// pbs_wave.h::pack_lwe_team states the operation and its exactness bound.  Two kernels per call:
//
// pack_transpose_kernel: lwe_in [groups][m][d+1] -> cols [groups][d+1][N], cols[g][i][j] = lwe_in[g][j][i] for j < m
// and 0 for m <= j < N (row d is the body polynomial sum_j b_j X^j).  32 x 32 tiles through LDS (33-word rows: no bank
// conflicts either way), 128-byte segments on both sides; grid (tiles over i, tiles over j, groups -- strided).
//
// pack_lwe_kernel: grid (output GLWE, run of key-row slices), x fastest, so that the teams in flight at one time are
// all the outputs of a few runs and read the same slices of the key while those are hot in the L2s.  A team sums its
// slices in LDS and adds the partial result to the pre-zeroed output with u32 atomic adds -- 64 consecutive words per
// wave instruction; wrapping addition is associative and commutative, so the bits do not depend on the order the
// teams arrive in.  Run 0 of an output also contributes the body row.
constexpr int kPackTile = 32;
// log_rep > 0 (the tree LUT's replicated layout): column j holds ciphertext j >> log_rep of the group, so that each of
// the m = N >> log_rep inputs fills 2^log_rep neighbouring coefficients -- the N-fold list is never written out.
__global__ void __launch_bounds__(256) pack_transpose_kernel(const u32* __restrict__ lwe_in, size_t groups, u32 m, u32 d,
                                                             u32 log_n, u32* __restrict__ cols, u32 log_rep) {
  __shared__ u32 tile[kPackTile][kPackTile + 1];
  const u32 N = 1u << log_n;
  const u32 width = d + 1;
  const u32 tx = threadIdx.x & (kPackTile - 1), ty = threadIdx.x / kPackTile;  // ty 0..7
  const u32 i0 = blockIdx.x * kPackTile, j0 = blockIdx.y * kPackTile;
  for (size_t g = blockIdx.z; g < groups; g += gridDim.z) {
    const u32* in = lwe_in + g * (size_t)m * width;
    u32* out = cols + g * (size_t)width * N;
#pragma unroll
    for (u32 t = 0; t < kPackTile; t += 8) {
      const u32 j = (j0 + ty + t) >> log_rep, i = i0 + tx;
      tile[ty + t][tx] = (j < m && i < width) ? in[(size_t)j * width + i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (u32 t = 0; t < kPackTile; t += 8) {
      const u32 i = i0 + ty + t, j = j0 + tx;  // j < N: N is a multiple of the tile
      if (i < width) out[(size_t)i * N + j] = tile[tx][ty + t];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------ tree LUT: the rotations' inputs
// The rotate kernels address sample r's ciphertext and test vector at r * stride: rotation r = (row, table, sub-table) of
// a tree-LUT level gets its own copy of the row's digit and -- at level 0 -- its own test vector, in the reserved
// workspace (capi.cpp::tfhe_tree_lut_batch_device).  One workgroup per rotation, grid-strided.
//
// tree_lut_expand_kernel: out [rows * per_row][words], out[r] = in[r / per_row]
__global__ void __launch_bounds__(256) tree_lut_expand_kernel(const u32* __restrict__ in, size_t count, size_t per_row, u32 words,
                                                              u32* __restrict__ out) {
  for (size_t r = blockIdx.x; r < count; r += gridDim.x) {
    const u32* src = in + (r / per_row) * words;
    u32* dst = out + r * words;
    for (u32 i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  }
}
// tree_lut_test_vectors_kernel: tv [rows][tables][subs][N], tv[row][t][h] = construct_test_from_lut(T[set][t][h B .. h B + B))
// (test_vector.rs:38-67: every value `rep` = N / B times, the first rep / 2 negated mod B, rotated left by rep / 2), B = 2^log_p,
// T = table + row * set_stride (0: one shared set), un-encoded like every clear test vector
__global__ void __launch_bounds__(256) tree_lut_test_vectors_kernel(const u32* __restrict__ table, size_t set_stride, size_t count,
                                                                    size_t per_row /* tables * subs */, u32 log_p, u32 log_n,
                                                                    u32* __restrict__ tv) {
  const u32 N = 1u << log_n, log_rep = log_n - log_p, mid = (1u << log_rep) >> 1;
  for (size_t r = blockIdx.x; r < count; r += gridDim.x) {
    const u32* lut = table + (r / per_row) * set_stride + ((r % per_row) << log_p);
    u32* dst = tv + r * N;
    for (u32 i = threadIdx.x; i < N; i += blockDim.x) {
      const u32 idx = (i + mid) & (N - 1u);
      u32 val = lut[idx >> log_rep];
      if (idx < mid && val != 0u) val = (1u << log_p) - val;
      dst[i] = val;
    }
  }
}

template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
pack_lwe_kernel(PbsParams P /* the KS decomposer */, const typename F::elem* __restrict__ tw,
                const typename F::elem* __restrict__ key, const u32* __restrict__ cols, u32 d, u32 slices,
                u32 slices_per_run, u32* glwe_out) {
  using C = TeamCfg<F, LOGN, K, 1>;
  constexpr int N = C::N;
  constexpr int G = C::G;
  constexpr int E = NttShape<LOGN, G>::kE;
  constexpr int T = NttShape<LOGN, G>::kThreads;
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  const u32 s0 = blockIdx.y * slices_per_run;
  const u32 s1 = s0 + slices_per_run < slices ? s0 + slices_per_run : slices;
  const u32* mine = cols + (size_t)blockIdx.x * ((size_t)d + 1) * N;
  pack_lwe_team<F, LOGN, K, G>(w, P, mine, d, blockIdx.y == 0 ? mine + (size_t)d * N : nullptr, key, s0, s1);
  u32* dst = glwe_out + ((size_t)blockIdx.x * (K + 1) + w.group()) * N;
  const int tid = w.tid();
#pragma unroll
  for (int r = 0; r < E; ++r) atomicAdd(&dst[r * T + tid], w.acc()[r * T + tid]);
}

// ------------------------------------------------------------------------------ CMUX tree / encrypted table lookup
// pbs_wave.h::cmux_tree_team states the operations.  One team per (tree, subtree) of a pass, tree = blockIdx.x >>
// log_subtrees; the team's LDS and registers are external_product_kernel's (one product at a time, x in c.acc(), the
// pending partial results in the team's slots of the workspace), so its residency is that kernel's.
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
cmux_tree_kernel(PbsParams P, const typename F::elem* __restrict__ tw, CmuxTreePass pass) {
  using C = TeamCfg<F, LOGN, K, 1>;
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  cmux_tree_team<F, LOGN, K, C::G>(w, P, pass, (size_t)(blockIdx.x >> pass.log_subtrees),
                                   blockIdx.x & ((1u << pass.log_subtrees) - 1u));
}

// ------------------------------------------------------------------------------ DEMUX tree / encrypted table update
// pbs_wave.h::demux_tree_team states the operations.  One team per (tree, root) of a pass, as in cmux_tree_kernel; the
// team's LDS is that kernel's (one product at a time, x in c.acc(), the parked nodes in the team's slots of the workspace).
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
demux_tree_kernel(PbsParams P, const typename F::elem* __restrict__ tw, DemuxTreePass pass) {
  using C = TeamCfg<F, LOGN, K, 1>;
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  demux_tree_team<F, LOGN, K, C::G>(w, P, pass, (size_t)(blockIdx.x >> pass.log_subtrees),
                                    blockIdx.x & ((1u << pass.log_subtrees) - 1u));
}

// ------------------------------------------------------------------------------ encrypted branching program
// pbs_wave.h::cmux_program_team states the operations.  One team per (query, part) of a pass; the team's LDS is
// cmux_tree_kernel's (one product at a time; acc stages the operand of a rotated node and the outputs' extraction).
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
cmux_program_kernel(PbsParams P, const typename F::elem* __restrict__ tw, CmuxProgramPass pass) {
  using C = TeamCfg<F, LOGN, K, 1>;
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  cmux_program_team<F, LOGN, K, C::G>(w, P, pass, (size_t)(blockIdx.x / pass.parts), blockIdx.x % pass.parts);
}

// dst row `row` = GLWE [k+1][N]: coefficient 0 of the body += factor[row] (the packing key's s_i g_l)
__global__ void packing_add_gadget_kernel(u32* pksk, size_t rows, u32 k, u32 log_n, const u32* __restrict__ factor) {
  for (size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x; row < rows; row += (size_t)gridDim.x * blockDim.x)
    pksk[(row * (k + 1) + k) << log_n] += factor[row];
}

// ------------------------------------------------------------------------------ GLWE key switch / automorphism
// glwe_switch.h::glwe_switch_team states the operation.  One team per ciphertext, one launch per call: no workspace, no
// memset, nothing but the team's own ciphertext is touched (glwe_out may be glwe_in).  The team's LDS and registers are
// pack_lwe_kernel's.
template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
glwe_switch_kernel(PbsParams P /* the KS decomposer */, const typename F::elem* __restrict__ tw,
                   const typename F::elem* __restrict__ key, const u32* glwe_in, u32 t_inv, u32 add_input, u32* glwe_out) {
  using C = TeamCfg<F, LOGN, K, 1>;
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  const size_t at = (size_t)blockIdx.x * (K + 1) * C::N;
  glwe_switch_team<F, LOGN, K, C::G>(w, P, glwe_in + at, t_inv, add_input, key, glwe_out + at);
}

// glwe_switch.h::automorphism_poly: the bare permutation, one workgroup per polynomial (grid-strided)
struct AutomorphismWorkgroup {
  __device__ u32 thread() const { return threadIdx.x; }
  __device__ u32 threads() const { return blockDim.x; }
  __device__ void barrier() const { __syncthreads(); }
  __device__ u32* lds() const { return reinterpret_cast<u32*>(g_smem); }
};
__global__ void __launch_bounds__(256) glwe_automorphism_kernel(const u32* in, size_t polys, u32 log_n, u32 t_inv, u32* out) {
  for (size_t p = blockIdx.x; p < polys; p += gridDim.x)
    automorphism_poly(AutomorphismWorkgroup(), in + (p << log_n), log_n, t_inv, out + (p << log_n));
}

// key [k l_ks][k+1][N]: the body of row i l_ks + l += from_polys[i] (coefficients in {-1, 0, 1}) times the gadget factor
// g_l = 2^(top - log_base (l + 1)); a -1 adds 0 - g_l
__global__ void __launch_bounds__(256) glwe_switch_add_gadget_kernel(u32* key, u32 k, u32 log_n, u32 levels, u32 log_base, u32 top,
                                                                     const i32* __restrict__ from_polys) {
  const size_t total = ((size_t)k * levels) << log_n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i >> log_n;
    const u32 j = (u32)(i & ((1u << log_n) - 1u));
    const u32 g = 1u << (top - log_base * ((u32)(row % levels) + 1u));
    key[((row * (k + 1) + k) << log_n) + j] += (u32)from_polys[((row / levels) << log_n) + j] * g;
  }
}

// ------------------------------------------------------------------------------ key switch
// out[b][c] = -sum_{i<big_n, l<levels} digit_l(lwe[b][i]) * ksk[i*levels + l][c];  out[b][n] += b
// Tiled as a wrapping-u32 GEMM: a workgroup owns kKsSamples samples x 128 output columns and walks
// key rows in chunks; digits of the chunk are produced once into LDS.  The key rows are staged through
// LDS as well, kKsKeyRows at a time and double-buffered: the four waves of a workgroup all need the same
// 128 columns of every row (they differ in the samples they own), and reading them straight from global
// memory quadrupled the L1 traffic -- 512 B per wave and row at ~75 cycles per row and ten waves per CU is
// more than the 64 B/clk a CU's vector L1 delivers, which is what bounded the kernel (1.30 ms against a
// 0.39 ms multiply-add floor at cfg2).  Small batches do not give enough (sample, column) tiles to fill
// 256 CUs, so the big_n mask words are also split over gridDim.z: with more than one split the partial
// sums go to the (pre-zeroed) output with u32 atomic adds -- wrapping addition is associative and
// commutative, the bits do not depend on the order.
constexpr int kKsSamples = 32;     // samples per workgroup
constexpr int kKsColsPerLane = 2;  // output columns per lane
constexpr int kKsCols = 64 * kKsColsPerLane;  // output columns per workgroup
constexpr int kKsWords = 8;        // mask words decomposed per chunk
constexpr int kKsPerThread = 8;    // samples per thread (kKsSamples / 4 waves)
constexpr int kKsKeyRows = 16;     // key rows staged in LDS per step (x 128 columns x 4 B = 8 KiB, two buffers)
constexpr int kKsLoads = kKsKeyRows * kKsCols / 256;  // key words each thread moves per step
// workgroups a launch should reach before the mask words stop being split over gridDim.z: 16 per CU
// (cfg2, batch 4096: 640 tiles -> 0.90 ms unsplit, 0.70 ms at 3 splits, 0.59 ms at 6; flat beyond)
constexpr unsigned kKsTargetWgs = 4096u;

__global__ void __launch_bounds__(256) key_switch_kernel(KsParams Kp, u32 big_n, u32 n,
                                                         const u32* __restrict__ lwe_in, size_t batch,
                                                         const u32* __restrict__ ksk,
                                                         u32* __restrict__ lwe_out, u32 words_per_split) {
  const u32 levels = Kp.levels;
  u32* dig = reinterpret_cast<u32*>(g_smem);                 // [kKsWords*levels][kKsSamples]
  u32* ktile = dig + (size_t)kKsWords * levels * kKsSamples;  // [2][kKsKeyRows][kKsCols]
  const int tx = (int)(threadIdx.x & 63u);
  const int ty = (int)(threadIdx.x >> 6);
  const size_t s0 = (size_t)blockIdx.y * kKsSamples;
  const u32 width = n + 1;
  const u32 col0 = blockIdx.x * kKsCols;
  u32 col[kKsColsPerLane];
  bool col_ok[kKsColsPerLane];
#pragma unroll
  for (int c = 0; c < kKsColsPerLane; ++c) {
    col[c] = col0 + c * 64 + tx;
    col_ok[c] = col[c] < width;
  }
  // staging slot of this thread: column lc of rows lr, lr + 2, ... of a step (a wave covers 64
  // consecutive columns of one row: coalesced)
  const u32 lc = threadIdx.x & (kKsCols - 1);
  const u32 lr = threadIdx.x / kKsCols;
  const bool lc_ok = col0 + lc < width;

  // 64-bit accumulators so that every multiply-add is ONE v_mad_u64_u32; only bits 31..0 are kept
  u64 acc[kKsColsPerLane][kKsPerThread];
#pragma unroll
  for (int c = 0; c < kKsColsPerLane; ++c)
#pragma unroll
    for (int s = 0; s < kKsPerThread; ++s) acc[c][s] = 0;

  const u32 w_begin = blockIdx.z * words_per_split;  // multiple of kKsWords
  const u32 w_end = (w_begin + words_per_split < big_n) ? w_begin + words_per_split : big_n;
  for (u32 w0 = w_begin; w0 < w_end; w0 += kKsWords) {
    const u32 rows = ((w_end - w0 < (u32)kKsWords) ? (w_end - w0) : (u32)kKsWords) * levels;
    const u32* krow = ksk + (size_t)w0 * levels * width + col0;
    u32 stage[kKsLoads];
    auto fetch = [&](u32 first_row) {  // rows first_row + lr + 2 i of this chunk -> registers
#pragma unroll
      for (int i = 0; i < kKsLoads; ++i) {
        const u32 r = first_row + lr + (256 / kKsCols) * i;
        stage[i] = (lc_ok && r < rows) ? krow[(size_t)r * width + lc] : 0u;
      }
    };
    fetch(0);
    // 256 threads decompose 32 samples x 8 words: thread -> (sample = tid / 8, word = tid % 8)
    {
      const int sl = (int)(threadIdx.x >> 3);
      const u32 wl = threadIdx.x & 7u;
      const size_t sample = s0 + sl;
      const u32 word = w0 + wl;
      u32 v = 0;
      if (sample < batch && word < w_end) v = lwe_in[sample * ((size_t)big_n + 1) + word];
      v = round_value(v, Kp.ignored_bits);
      u32 carry = 0;
      for (u32 t = 0; t < levels; ++t) {  // LSB -> MSB, level index counts from the MSB
        const u32 d = decompose_limb(v, Kp.first_shift + Kp.log_base * t, Kp.log_base, carry);
        dig[(wl * levels + (levels - 1 - t)) * kKsSamples + sl] = d;
      }
    }
    // one barrier per step: a step writes buffer (step & 1), which was last read two steps ago, and
    // every thread has passed the barrier of the step in between since (the first barrier of a chunk
    // also publishes the digits; the chunk's last one, below, protects them from the next chunk)
    for (u32 r0 = 0, step = 0; r0 < rows; r0 += kKsKeyRows, ++step) {
      u32* kt = ktile + (step & 1u) * (kKsKeyRows * kKsCols);
#pragma unroll
      for (int i = 0; i < kKsLoads; ++i) kt[(lr + (256 / kKsCols) * i) * kKsCols + lc] = stage[i];
      __syncthreads();
      if (r0 + kKsKeyRows < rows) fetch(r0 + kKsKeyRows);  // in flight while this step computes
      const u32 here = rows - r0 < (u32)kKsKeyRows ? rows - r0 : (u32)kKsKeyRows;
#pragma unroll 4
      for (u32 r = 0; r < here; ++r) {
        u32 kv[kKsColsPerLane];
#pragma unroll
        for (int c = 0; c < kKsColsPerLane; ++c) kv[c] = kt[r * kKsCols + c * 64 + tx];
        const u32* d = dig + (r0 + r) * kKsSamples + ty * kKsPerThread;
#pragma unroll
        for (int s = 0; s < kKsPerThread; ++s) {
          const u32 ds = d[s];  // same address in every lane of the wave: LDS broadcast
#pragma unroll
          for (int c = 0; c < kKsColsPerLane; ++c) acc[c][s] = (u64)ds * kv[c] + acc[c][s];
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int c = 0; c < kKsColsPerLane; ++c) {
    if (!col_ok[c]) continue;
#pragma unroll
    for (int s = 0; s < kKsPerThread; ++s) {
      const size_t sample = s0 + ty * kKsPerThread + s;
      if (sample >= batch) continue;
      u32 v = 0u - (u32)acc[c][s];
      if (col[c] == n && blockIdx.z == 0) v += lwe_in[sample * ((size_t)big_n + 1) + big_n];
      if (gridDim.z == 1) lwe_out[sample * width + col[c]] = v;
      else atomicAdd(&lwe_out[sample * width + col[c]], v);
    }
  }
}

// ------------------------------------------------------------------------------ key switch on the matrix cores
// The same sum as key_switch_kernel through v_mfma_i32_32x32x32_i8 over the prepared key of ks_matrix.h, which states
// the layout and why the bits are the same.  One thread per (super-block, level, column tile, lane): the 16 key words
// of the lane's fragment, split into their four byte planes.
__global__ void __launch_bounds__(256) ksk_prepare_matrix_kernel(KsmLayout lo, const u32* __restrict__ ksk,
                                                                 unsigned char* __restrict__ prepared) {
  const size_t total = (size_t)lo.sblocks * lo.levels * lo.col_tiles * 64;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const u32 lane = (u32)(i & 63u);
    size_t f = i >> 6;
    const u32 ct = (u32)(f % lo.col_tiles);
    f /= lo.col_tiles;
    const u32 level = (u32)(f % lo.levels);
    const u32 sb = (u32)(f / lo.levels);
    u32 planes[kKsmPlanes][4];
    ksm_prepare_lane(lo, ksk, sb, level, ct, lane, planes);
#pragma unroll
    for (u32 p = 0; p < kKsmPlanes; ++p)  // 16-byte aligned: fragments are 1 KiB, a lane's share 16 bytes
      *reinterpret_cast<uint4*>(prepared + ksm_fragment(lo, sb, level, ct, p) + (size_t)lane * 16) =
          make_uint4(planes[p][0], planes[p][1], planes[p][2], planes[p][3]);
  }
}

// A workgroup is four waves, each with its own tile of 32 samples and the same kKsmColTiles column tiles (the waves
// fetch the same key fragments: one trip to L2 serves four).  Per super-block a lane loads the 16 mask words of its
// sample that its half of the MFMA's K covers, and per level -- LSB first, as the carry chain runs -- decomposes them
// into its own A fragment; K is walked in that order, (super-block, level from the last down).  Each (column tile,
// plane) keeps an int32 accumulator tile; ksm_admitted (checked by the launcher) bounds their sums, so they are folded
// once at the end: total = sum_j plane_j << 8j in wrapping u32.  gridDim.z splits the super-blocks as
// key_switch_kernel splits the mask words: partial sums are added to the pre-zeroed output with atomics.
// workgroups a launch should reach before the super-blocks stop being split over gridDim.z: four per CU
constexpr unsigned kKsmTargetWgs = 1024u;
// smallest batch TFHE_KS_PATH_AUTO sends here.  Below one tile of 32 samples most of every MFMA is padding, and it still
// wins: 0.019 ms against 0.055 ms at batch 1, cfg1 and cfg2 alike (profiles/key_switch_matrix_ab.txt), so: every batch
constexpr size_t kKsMatrixMinBatch = 1;
__global__ void __launch_bounds__(256, 2) key_switch_matrix_kernel(KsParams Kp, KsmLayout lo, const u32* __restrict__ lwe_in,
                                                                size_t batch, const uint4* __restrict__ prepared,
                                                                u32* __restrict__ lwe_out, u32 sblocks_per_split) {
  const u32 lane = threadIdx.x & 63u;
  const u32 r = lane & 31u, h = lane >> 5;
  const size_t sample0 = ((size_t)blockIdx.y * 4 + (threadIdx.x >> 6)) * kKsmSamples;
  if (sample0 >= batch) return;  // no barrier below: a wave without samples leaves
  const size_t sample = sample0 + r;
  const bool sample_ok = sample < batch;
  const size_t stride = (size_t)lo.big_n + 1;
  const u32* row = lwe_in + (sample_ok ? sample : sample0) * stride;
  const u32 ct0 = blockIdx.x * kKsmColTiles;

  i32x16 acc[kKsmColTiles][kKsmPlanes];
#pragma unroll
  for (u32 c = 0; c < kKsmColTiles; ++c)
#pragma unroll
    for (u32 p = 0; p < kKsmPlanes; ++p)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[c][p][e] = 0;

  const u32 sb_begin = blockIdx.z * sblocks_per_split;
  const u32 sb_end = sb_begin + sblocks_per_split < lo.sblocks ? sb_begin + sblocks_per_split : lo.sblocks;
  for (u32 sb = sb_begin; sb < sb_end; ++sb) {
    u32 v[16], carry[16];
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
      const u32 word = sb * kKsmWords + h * 16 + j;
      const u32 x = row[word < lo.big_n ? word : 0u];  // always in bounds; a padding word counts as zero, which
      v[j] = round_value((sample_ok && word < lo.big_n) ? x : 0u, Kp.ignored_bits);  // rounds and decomposes to zeros
      carry[j] = 0;
    }
    for (u32 t = 0; t < Kp.levels; ++t) {  // LSB -> MSB, level index counts from the MSB
      const u32 level = Kp.levels - 1 - t;
      const uint4* frag = prepared + ksm_fragment(lo, sb, level, ct0, 0) / 16 + lane;
      uint4 b[kKsmColTiles][kKsmPlanes];
#pragma unroll
      for (u32 c = 0; c < kKsmColTiles; ++c)
#pragma unroll
        for (u32 p = 0; p < kKsmPlanes; ++p) b[c][p] = frag[(c * kKsmPlanes + p) * 64];
      u32 digits[4];
      ksm_digit_fragment(v, carry, Kp.first_shift + Kp.log_base * t, Kp.log_base, digits);
      const i32x4 a = {(i32)digits[0], (i32)digits[1], (i32)digits[2], (i32)digits[3]};
#pragma unroll
      for (u32 c = 0; c < kKsmColTiles; ++c)
#pragma unroll
        for (u32 p = 0; p < kKsmPlanes; ++p) {
          const i32x4 bf = {(i32)b[c][p].x, (i32)b[c][p].y, (i32)b[c][p].z, (i32)b[c][p].w};
          acc[c][p] = mfma_i32_32x32x32_i8(a, bf, acc[c][p]);
        }
    }
  }

#pragma unroll
  for (u32 c = 0; c < kKsmColTiles; ++c) {
    const u32 col = (ct0 + c) * kKsmCols + r;
    if (col >= lo.width) continue;
#pragma unroll
    for (u32 e = 0; e < 16; ++e) {
      const size_t s = sample0 + (e & 3u) + 8 * (e >> 2) + 4 * h;
      if (s >= batch) continue;
      u32 out = 0u - ksm_fold((u32)acc[c][0][e], (u32)acc[c][1][e], (u32)acc[c][2][e], (u32)acc[c][3][e]);
      if (col == lo.width - 1 && blockIdx.z == 0) out += lwe_in[s * stride + lo.big_n];
      if (gridDim.z == 1) lwe_out[s * lo.width + col] = out;
      else atomicAdd(&lwe_out[s * lo.width + col], out);
    }
  }
}

// ------------------------------------------------------------------------------ elementwise
__global__ void decompose_words_kernel(u32 log_base, u32 levels, u32 ignored_bits, u32 first_shift,
                                       const u32* __restrict__ values, size_t count,
                                       u32* __restrict__ digits) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (size_t)gridDim.x * blockDim.x) {
    const u32 v = round_value(values[i], ignored_bits);
    u32 carry = 0;
    for (u32 t = 0; t < levels; ++t)
      digits[i * levels + (levels - 1 - t)] = decompose_limb(v, first_shift + log_base * t, log_base, carry);
  }
}

// glwe [batch][polys][N] -> digits [batch][polys*levels][N]
__global__ void decompose_glwe_kernel(u32 log_base, u32 levels, u32 ignored_bits, u32 first_shift,
                                      u32 polys, u32 n_coeff, const u32* __restrict__ glwe,
                                      size_t total /* batch*polys*N */, u32* __restrict__ digits) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t poly = i / n_coeff;  // global polynomial index = b*polys + p
    const u32 j = (u32)(i % n_coeff);
    const u32 v = round_value(glwe[i], ignored_bits);
    u32 carry = 0;
    for (u32 t = 0; t < levels; ++t)
      digits[(poly * levels + (levels - 1 - t)) * n_coeff + j] =
          decompose_limb(v, first_shift + log_base * t, log_base, carry);
  }
}

__global__ void switch_modulus_kernel(const u32* __restrict__ values, size_t count, u32 log_from,
                                      u32 log_to, u32* __restrict__ out) {
  // utils.rs:13-33
  const u32 sh = log_from - log_to;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (size_t)gridDim.x * blockDim.x) {
    u32 v = values[i];
    if (sh == 0) {
      // divisor 1: rational = v, fractional = 0
    } else {
      v = (v >> sh) + ((v >> (sh - 1)) & 1u);
    }
    out[i] = (log_to >= 32) ? v : (v & ((1u << log_to) - 1u));
  }
}

__global__ void glwe_mul_monomial_kernel(u32 log_n, u32 polys, const u32* __restrict__ glwe,
                                         size_t total, const i64* __restrict__ monomial_index,
                                         u32* __restrict__ out) {
  const u32 N = 1u << log_n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t poly = i >> log_n;
    const u32 j = (u32)(i & (N - 1));
    // `monomial_index as usize % (2*n)` (utils.rs:186): two's complement residue mod 2N
    const u32 m = (u32)((u64)monomial_index[poly / polys] & (u64)(2 * N - 1));
    const u32 deg = m & (N - 1);
    const u32 flip = (m >> log_n) & 1u;
    const u32 v = glwe[(poly << log_n) + ((j - deg) & (N - 1))];
    out[i] = (flip ^ (u32)(j < deg)) ? (0u - v) : v;
  }
}

__global__ void sample_extract_kernel(u32 log_n, u32 k, const u32* __restrict__ glwe, size_t batch,
                                      u32 sample_index, u32* __restrict__ lwe_out) {
  // bootstrapping.rs:122-156: per mask polynomial p[idx], p[idx-1], ..., p[0], -p[N-1], ..., -p[idx+1]
  const u32 N = 1u << log_n;
  const size_t width = (size_t)k * N + 1;
  const size_t total = batch * width;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / width;
    const size_t x = i % width;
    const u32* ct = glwe + b * (size_t)(k + 1) * N;
    u32 v;
    if (x == (size_t)k * N) {
      v = ct[(size_t)k * N + sample_index];
    } else {
      const u32 p = (u32)(x >> log_n);
      const u32 pos = (u32)(x & (N - 1));
      v = (pos <= sample_index) ? ct[(size_t)p * N + (sample_index - pos)]
                                : (0u - ct[(size_t)p * N + (N + sample_index - pos)]);
    }
    lwe_out[i] = v;
  }
}

// out = c0*ct0 + c1*ct1, plus b_add on the last word of every ciphertext of words_per_ct words
// (words_per_ct == 0: no constant term)
__global__ void lwe_linear_kernel(u32 c0, const u32* ct0, u32 c1, const u32* ct1, size_t words,
                                  size_t words_per_ct, u32 b_add, u32* out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words;
       i += (size_t)gridDim.x * blockDim.x) {
    u32 v = c0 * ct0[i] + (ct1 ? c1 * ct1[i] : 0u);
    if (words_per_ct && (i % words_per_ct) == words_per_ct - 1) v += b_add;
    out[i] = v;
  }
}

// ------------------------------------------------------------------------------ dense layer
// lwe_dense.h::dense_tile states the operations and the tiling; this is its workgroup context on the device.
struct DenseWorkgroup {
  __device__ u32 thread() const { return threadIdx.x; }
  __device__ u32 block_x() const { return blockIdx.x; }
  __device__ u32 block_y() const { return blockIdx.y; }
  __device__ u32 block_z() const { return blockIdx.z; }
  __device__ void barrier() const { __syncthreads(); }
  __device__ u32* lds() const { return reinterpret_cast<u32*>(g_smem); }
  __device__ void atomic_add(u32* p, u32 v) const { atomicAdd(p, v); }
};
__global__ void __launch_bounds__(kDenseThreads) lwe_dense_kernel(DenseArgs a) { dense_tile(DenseWorkgroup(), a); }
// out [count][words], out[r] = in[r % period]: bootstrap r = (query, neuron) of a fused layer gets neuron r % O's test vector
__global__ void __launch_bounds__(256) dense_tile_rows_kernel(const u32* __restrict__ in, size_t period, size_t count, u32 words,
                                                              u32* __restrict__ out) {
  for (size_t r = blockIdx.x; r < count; r += gridDim.x) {
    const u32* src = in + (r % period) * words;
    u32* dst = out + r * words;
    for (u32 i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  }
}

// ------------------------------------------------------------------------------ digit extraction
// lwe_extract.h::extract_step states the step; this is its thread context on the device.
struct ExtractThread {
  __device__ size_t index() const { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }
  __device__ size_t threads() const { return (size_t)gridDim.x * blockDim.x; }
};
__global__ void __launch_bounds__(kExtractThreads) extract_step_kernel(ExtractStepArgs a) { extract_step(ExtractThread(), a); }

// ------------------------------------------------------------------------------ radix integers
// radix.h::radix_glue states the launch between two bootstrap levels; this is its thread context on the device.
struct RadixThread {
  __device__ size_t index() const { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }
  __device__ size_t threads() const { return (size_t)gridDim.x * blockDim.x; }
};
__global__ void __launch_bounds__(kRadixThreads) radix_glue_kernel(RadixGlueArgs a) { radix_glue(RadixThread(), a); }

// ------------------------------------------------------------------------------ seeded ciphertexts
// seeded.h::seeded_expand / seeded_compress state the launches; this is their workgroup context on the device.  V: words
// per store (4 where rows, masks and both pointers are 16-byte aligned).
struct SeededWorkgroup {
  u32* lds_;
  __device__ u32 thread() const { return threadIdx.x; }
  __device__ size_t block() const { return blockIdx.x; }
  __device__ size_t blocks() const { return gridDim.x; }
  __device__ void barrier() const { __syncthreads(); }
  __device__ u32* lds() const { return lds_; }
};
template <int V>
__global__ void __launch_bounds__(kSeededThreads) seeded_expand_kernel(SeededRowsArgs a) {
  __shared__ __attribute__((aligned(16))) u32 stage[kSeededLdsWords];
  seeded_expand<V>(SeededWorkgroup{stage}, a);
}
template <int V>
__global__ void __launch_bounds__(kSeededThreads) seeded_compress_kernel(SeededRowsArgs a) {
  seeded_compress<V>(SeededWorkgroup{nullptr}, a);
}

// ------------------------------------------------------------------------------ multi-value bootstrap
// multi_value.h::sparse_extract_tile states the per-table step; this is its workgroup context on the device.  The
// pointers arrive as kernel arguments of their own, not in the struct: only there does __restrict__ tell the compiler
// that the stores to out cannot touch positions or coeffs, which is what lets it read both with scalar loads.
struct SparseWorkgroup {
  __device__ u32 thread() const { return threadIdx.x; }
  __device__ u32 block_x() const { return blockIdx.x; }
  __device__ u32 block_y() const { return blockIdx.y; }
  __device__ void barrier() const { __syncthreads(); }
  __device__ u32* lds() const { return reinterpret_cast<u32*>(g_smem); }
};
__global__ void __launch_bounds__(kSparseThreads)
glwe_sparse_extract_kernel(const u32* __restrict__ glwe, const u32* __restrict__ positions, const i32* __restrict__ coeffs,
                           u32* __restrict__ out, size_t set_stride, u32 log_n, u32 k, u32 terms, u32 tables, u32 tables_per_run) {
  const SparseExtractArgs a{glwe, positions, coeffs, out, set_stride, log_n, k, terms, tables, tables_per_run};
  sparse_extract_tile(SparseWorkgroup(), a);
}
// coeffs [rows][B + 1] = the coefficients of (1 - X) construct_test_from_lut(luts[row]), luts [rows][B]
__global__ void __launch_bounds__(256) multi_value_coefficients_kernel(const u32* __restrict__ luts, size_t rows, u32 log_p,
                                                                       i32* __restrict__ coeffs) {
  const u32 terms = (1u << log_p) + 1u;
  const size_t total = rows * terms;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    coeffs[i] = (i32)multi_value_coefficient(luts + ((i / terms) << log_p), (u32)(i % terms), log_p);
}
// what a context's multi-value calls share: the accumulator (0, .., 0, kappa (1 + X + .. + X^(N-1))) and the B + 1 positions
__global__ void __launch_bounds__(256) multi_value_constants_kernel(u32 log_p, u32 log_n, u32 k, u32 kappa, u32* __restrict__ acc,
                                                                    u32* __restrict__ positions) {
  const u32 acc_words = (k + 1u) << log_n, body = k << log_n, terms = (1u << log_p) + 1u;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < acc_words; i += gridDim.x * blockDim.x) acc[i] = i >= body ? kappa : 0u;
  for (u32 m = blockIdx.x * blockDim.x + threadIdx.x; m < terms; m += gridDim.x * blockDim.x)
    positions[m] = multi_value_position(m, log_p, log_n);
}
// a caller's positions come from host memory: up to kSparsePositionsPerLaunch of them travel as kernel arguments, so that a
// captured call carries them in the graph
constexpr u32 kSparsePositionsPerLaunch = 64;
struct SparsePositions {
  u32 v[kSparsePositionsPerLaunch];
};
__global__ void __launch_bounds__(64) sparse_positions_kernel(SparsePositions p, u32 count, u32* __restrict__ dst) {
  if (threadIdx.x < count) dst[threadIdx.x] = p.v[threadIdx.x];
}

// ------------------------------------------------------------------------------ encrypted convolution
// glwe_conv.h states the operation and its exactness bound.  Two kernels:
//
// conv_weights_kernel: once per weight set, the forward transforms of the O * C weight polynomials into the form the
// multiply-accumulate consumes; one polynomial per group of G waves, as in bsk_prepare_kernel.
//
// glwe_conv_kernel: one team per (query, output), output fastest, so that the teams in flight at one time read the
// prepared ciphertexts of a few queries and all weight sets while those are hot in the L2s.  The ciphertext spectra of
// the call come from bsk_prepare_kernel, in the layout of the context's k.
template <class F, int LOGN>
__global__ void __launch_bounds__(256) conv_weights_kernel(const typename F::elem* __restrict__ tw, const i32* __restrict__ polys,
                                                          size_t poly_count, typename F::elem* __restrict__ spectra) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr int G = GroupOf<F, LOGN>::value;
  elem* twl = reinterpret_cast<elem*>(g_smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, G>(twl, tw, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  const int group = (int)(threadIdx.x / (64u * G));
  const int groups = (int)(blockDim.x / (64u * G));
  // (G > 1: the transform holds workgroup barriers, so a group past the end redoes the last polynomial)
  size_t poly = (size_t)blockIdx.x * groups + group;
  if (poly >= poly_count) {
    if (G == 1) return;
    poly = poly_count - 1;
  }
  DeviceWave<elem, G> w;
  w.group_ = 0;
  w.group_stride_ = 0;
  w.buffer_bytes_ = 0;
  w.acc_words_ = 0;
  w.team_base_ = nullptr;
  w.tw_ = twl;
  w.twg_ = tw;
  w.scratch_ = reinterpret_cast<elem*>(g_smem + twiddle_bytes<F, LOGN>() + (size_t)group * N * 8);
  w.acc_ = nullptr;
  conv_weights_wave<F, LOGN, G>(w, polys + poly * N, spectra + poly * (N >> F::kLogShrink));
}

template <class F, int LOGN, int K>
__global__ void __launch_bounds__((TeamCfg<F, LOGN, K, 1>::kThreads), (TeamCfg<F, LOGN, K, 1>::kMinWaves))
glwe_conv_kernel(const typename F::elem* __restrict__ tw, GlweConvArgs a) {
  using C = TeamCfg<F, LOGN, K, 1>;
  auto w = make_wave<F, LOGN, K, 1>(g_smem, tw);
  glwe_conv_team<F, LOGN, K, C::G>(w, a, (size_t)(blockIdx.x / a.outputs), blockIdx.x % a.outputs);
}

// lwe_out [batch][count][k N + 1]: sample_extract_kernel's words at indices[0 .. count) of every GLWE
__global__ void sample_extract_indices_kernel(u32 log_n, u32 k, const u32* __restrict__ glwe, size_t batch,
                                              const u32* __restrict__ indices, size_t count, u32* __restrict__ lwe_out) {
  const u32 N = 1u << log_n;
  const size_t width = (size_t)k * N + 1;
  const size_t total = batch * count * width;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / width;
    const size_t x = i % width;
    const u32 sample_index = indices[row % count] & (N - 1u);  // (the host has refused indices >= N: never out of the GLWE)
    const u32* ct = glwe + (row / count) * (size_t)(k + 1) * N;
    u32 v;
    if (x == (size_t)k * N) {
      v = ct[(size_t)k * N + sample_index];
    } else {
      const u32 p = (u32)(x >> log_n);
      const u32 pos = (u32)(x & (N - 1));
      v = (pos <= sample_index) ? ct[(size_t)p * N + (sample_index - pos)] : (0u - ct[(size_t)p * N + (N + sample_index - pos)]);
    }
    lwe_out[i] = v;
  }
}

// ------------------------------------------------------------------------------ encryption side
// dst[row][j] = body_in[row][j] +/- sum_i masks[row][i] (*) sk[i]: one GLWE row [k+1][N] per group
// of G waves, 4/G rows per workgroup.  Encrypt (glwe.rs:190-209): body_in holds the caller's error
// samples, dst = the body itself.  Decrypt (glwe.rs:245-265): dst = plaintext rows, negate = 1.
template <class F, int LOGN>
__global__ void __launch_bounds__(256) glwe_body_kernel(const typename F::elem* __restrict__ tw, u32 k,
                                                       const u32* rows, size_t row_count,
                                                       const u32* __restrict__ sk, u32* dst,
                                                       size_t dst_stride, u32 negate,
                                                       typename F::elem n_inv) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr int G = GroupOf<F, LOGN>::value;
  elem* twl = reinterpret_cast<elem*>(g_smem);
  ntt_stage_twiddles<LOGN - F::kLogShrink, G>(twl, tw, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  const int group = (int)(threadIdx.x / (64u * G));
  const int groups = (int)(blockDim.x / (64u * G));
  // G > 1: the transforms contain workgroup barriers, so a group past the end redoes the last row
  // (same values to the same addresses) instead of leaving -- as in bsk_prepare_kernel
  size_t row = (size_t)blockIdx.x * groups + group;
  bool live = true;
  if (row >= row_count) {
    if (G == 1) return;
    row = row_count - 1;
    live = false;
  }
  DeviceWave<elem, G> w;
  w.group_ = 0;
  w.group_stride_ = 0;
  w.buffer_bytes_ = 0;
  w.acc_words_ = 0;
  w.team_base_ = nullptr;
  w.tw_ = twl;
  w.twg_ = tw;
  w.scratch_ = reinterpret_cast<elem*>(g_smem + twiddle_bytes<F, LOGN>() + (size_t)group * N * 8);
  w.acc_ = nullptr;
  const u32* masks = rows + row * (size_t)(k + 1) * N;
  const u32* body = masks + (size_t)k * N;
  u32* d = dst + row * dst_stride;
  auto out = [&](int j, u32 dot) {
    // body[j] is read before d[j] is written by the same lane, so d may alias body
    const u32 b = body[j];
    if (live) d[j] = negate ? b - dot : b + dot;
  };
  glwe_mask_dot_key<F, LOGN, G>(w, k, masks, sk, n_inv, out);
}

// dst[row] = lwe[row][n] +/- <lwe[row][0..n), sk> (+ plaintext[row]): one LWE row per wavefront.
// Encrypt (lwe.rs:117-160, and the rows of generate_ksk key_switching.rs:41-45): the b slot holds
// the caller's error sample, dst = the b slot.  Decrypt (lwe.rs:162-173): negate = 1.
__global__ void __launch_bounds__(256) lwe_body_kernel(const u32* rows, size_t row_count, u32 n,
                                                      const u32* __restrict__ sk,
                                                      const u32* __restrict__ plaintext, u32* dst,
                                                      size_t dst_stride, u32 negate) {
  const size_t row = (size_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;
  if (row >= row_count) return;
  const u32 lane = threadIdx.x & 63u;
  const u32* ct = rows + row * ((size_t)n + 1);
  u32 dot = 0;
  for (u32 j = lane; j < n; j += 64u) dot += ct[j] * sk[j];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
  if (lane == 0) {
    const u32 b = ct[n];
    u32 v = negate ? b - dot : b + dot;
    if (plaintext) v += plaintext[row];
    dst[row * dst_stride] = v;
  }
}

// ggsw.rs:96-103: row = poly_index*levels + level of GGSW g gets
// messages[g] * 2^{gadget_top - log_base*(level+1)} added to coefficient 0 of polynomial poly_index
// (after the zero encryption was formed from the unmodified masks); gadget_top =
// log_base*floor(32/log_base) for the reference's literal decomposer
__global__ void ggsw_add_gadget_kernel(u32* ggsw, size_t ggsw_count, u32 k, u32 log_n, u32 levels,
                                       u32 log_base, u32 gadget_top, const u32* __restrict__ messages) {
  const size_t rows = (size_t)(k + 1) * levels;
  const size_t total = ggsw_count * rows;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t g = i / rows;
    const u32 row = (u32)(i % rows);
    const u32 poly_index = row / levels, level = row % levels;
    const u32 factor = messages[g] * (1u << (gadget_top - log_base * (level + 1)));
    ggsw[(((g * rows + row) * (k + 1)) + poly_index) << log_n] += factor;
  }
}

// HBM roofline probe: 16-byte-per-lane stream copy (the "float4 copy" of MI355X_MICROARCH.md).
// A workgroup moves one contiguous 16 KiB piece: every lane issues its 4 loads before the first
// store, so 64 B per lane are in flight; loads and stores are non-temporal (nothing is reused).
constexpr int kCopyUnroll = 4;
typedef unsigned int copy_vec4 __attribute__((ext_vector_type(4)));  // 16 bytes, what the builtins accept
__global__ void __launch_bounds__(256) stream_copy_kernel(const copy_vec4* __restrict__ src,
                                                         copy_vec4* __restrict__ dst, size_t count) {
  const size_t base = (size_t)blockIdx.x * (256 * kCopyUnroll) + threadIdx.x;
  copy_vec4 v[kCopyUnroll];
#pragma unroll
  for (int i = 0; i < kCopyUnroll; ++i)
    if (base + (size_t)i * 256 < count) v[i] = __builtin_nontemporal_load(&src[base + (size_t)i * 256]);
#pragma unroll
  for (int i = 0; i < kCopyUnroll; ++i)
    if (base + (size_t)i * 256 < count) __builtin_nontemporal_store(v[i], &dst[base + (size_t)i * 256]);
}

inline int grid_for(size_t work, int block) {
  size_t g = (work + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CUs x 8: grid-stride the rest
  if (g == 0) g = 1;
  return (int)g;
}

// Dynamic LDS above 64 KiB has to be enabled per kernel; done once per kernel and device (the
// attribute call is not something to repeat on every launch of a short kernel).  `done` is a bit
// mask over devices owned by the calling launcher, which is a distinct function (and so a distinct
// flag) per template instantiation; two host threads racing here both set the same attribute to
// the same value, which is harmless.
template <typename Kern>
hipError_t allow_lds(Kern kern, size_t bytes, std::atomic<unsigned long long>& done) {
  if (bytes <= 64 * 1024) return hipSuccess;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const unsigned long long bit = 1ull << dev;
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

// How a batch's blind rotations go out (launch_blind_rotate).
//   chunk     samples per group of launches
//   segments  launches per rotation: each walks key rows [i0, i1) only and parks the accumulators in global memory
//   streams   2: the two halves of a chunk go out on two streams, segment by segment in turn
// Why.  A team reads GGSW_i once per iteration (cfg2: 197 KB, 124 MB per rotation; the reference's defaults: 442 KB,
// 319 MB; N = 2048 with k = 2: 1.2 MB, 743 MB) and the complex transform's kernels draw 13-15 TB/s of it: that is L2
// bandwidth, and only while the teams that run at the same time read the SAME rows.  A launch of 4,096 samples is four
// rounds of the 1,024 teams the chip holds, and the dispatcher refills them one by one: teams of different rounds are at
// different iterations, most of the key is in use somewhere, and it comes from the Infinity Cache -- or, when it is larger
// than that (> 256 MiB), from HBM, again and again (PMC, cfg3: 258 GB per launch = 4 TB/s).  Round 2 kept launches short
// for that reason (4,096 samples: 109 k PBS/s at cfg2 against 75 k in one launch of 131,072).  Round 3 blocks the key
// instead (profiles/r03_kernel_ab.txt):
//   - SEGMENT launches: all teams of a launch, whatever their round, read the same slice of the key; a slice of a few MB
//     stays in the L2s.  Batch 4,096 on one stream: cfg3 62.2 k -> 71.2 k PBS/s from 32 segments on, cfg5 18.8 k -> 20.95 k
//     from 4 on (slices of <= 186 MB: the Infinity Cache holds them; no more from smaller ones), cfg2 and cfg1 (124 and
//     33 MB: they fit as they are) nothing: what the slices gain, every launch's tail -- the chip draining while the last
//     teams finish -- takes back.
//   - TWO STREAMS: the halves of the batch alternate, so one half's tail is filled by the other half's next launch.
//     Batch 4,096 with slices of 2 MiB: cfg2 117.6 k -> 125.2 k, cfg3 71.2 k -> 77.9 k, cfg1 358 k -> 387 k; it pays
//     as soon as the batch exceeds the teams the chip holds at once (at exactly that many it loses 2-4 %); three and
//     four streams add nothing; cfg5's 12-wave teams (one per CU) gain nothing either.
//   - with L2-sized slices launches can be LONG: cfg4's 131,072: 118.3 k in launches of 4,096 -> 128-130 k in one group.
//   (Measured and dropped: the same blocking inside ONE persistent launch -- teams that are never re-dispatched never
//   re-synchronise, 48 k at cfg3.)
// Hence, at N <= 1024: batches above what the chip holds at once go out in groups of up to 131,072 samples over key slices
// of half an L2 (l2_key_slice: 2 MiB on gfx950), on two streams; smaller ones in one launch.  That holds for every field (two streams + slices at batch 4,096:
// fp64-p49 at the reference's defaults 54.2 k -> 60.7 k PBS/s, Goldilocks at cfg2 29.2 k -> 30.8 k, fp64-p42 at cfg2 75.6 k
// -> 77.0 k).  At N = 2048: slices of 128 MiB if the key exceeds the Infinity Cache, one stream; the complex transform's
// long batches in groups of 16,384.  Without a place to park accumulators (state == nullptr): whole rotations, 4,096
// samples per launch for the complex transform (round 2: 109 k against 75 k PBS/s in one launch of 131,072), one launch
// for the prime fields (VALU-bound, they lose 2.5 % to launch boundaries).
// At least 4 iterations per segment.  TFHE_BR_CHUNK, TFHE_BR_SEGMENTS and TFHE_BR_STREAMS override (tests, sweeps).
struct BlindRotatePlan {
  size_t chunk;
  u32 segments;
  int streams;
};
inline long env_number(const char* name) {
  const char* env = std::getenv(name);
  const long v = env ? std::atol(env) : 0;
  return v > 0 ? v : 0;
}
constexpr int kMaxDevices = 64;
inline int current_device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  return dev;
}
// The key slice a segment launch walks: HALF of one L2 of the current device (an XCD's L2 on gfx950: 4 MiB, so 2 MiB -- the
// size the sweeps of round 3 settled on: the other half holds what the teams stream beside the key), asked once per device.
inline size_t l2_key_slice() {
  static std::atomic<size_t> cached[kMaxDevices];
  const int dev = current_device_slot();
  size_t slice = cached[dev].load(std::memory_order_acquire);
  if (slice == 0) {
    int l2 = 0;
    if (hipDeviceGetAttribute(&l2, hipDeviceAttributeL2CacheSize, dev) != hipSuccess || l2 <= 0) l2 = 4 << 20;
    slice = (size_t)l2 / 2;
    if (slice < ((size_t)1 << 20)) slice = (size_t)1 << 20;
    if (slice > ((size_t)16 << 20)) slice = (size_t)16 << 20;
    cached[dev].store(slice, std::memory_order_release);
  }
  return slice;
}
template <class F>
inline BlindRotatePlan blind_rotate_plan(size_t batch, bool can_park, bool have_side, u32 n, size_t key_bytes, u32 log_n,
                                         size_t resident_samples) {
  static const long env_chunk = env_number("TFHE_BR_CHUNK"), env_segments = env_number("TFHE_BR_SEGMENTS"),
                    env_streams = env_number("TFHE_BR_STREAMS");
  BlindRotatePlan plan{F::kLogShrink ? (size_t)4096 : (size_t)1 << 20, 1u, 1};
  if (can_park) {
    const bool fits = key_bytes <= ((size_t)224 << 20);  // the Infinity Cache, with room for the accumulators
    size_t slice = 0;
    if (log_n >= 11) {
      slice = fits ? 0 : (size_t)128 << 20;
      if (F::kLogShrink && batch >= 16384) plan.chunk = 16384;
    } else if (batch > resident_samples) {
      slice = l2_key_slice();
      plan.chunk = 131072;
      plan.streams = have_side ? 2 : 1;
    } else {
      plan.chunk = batch ? batch : 1;
    }
    if (env_streams) plan.streams = have_side && env_streams >= 2 ? 2 : 1;
    if (plan.streams == 2 && slice == 0) slice = l2_key_slice();
    plan.segments = slice ? (u32)((key_bytes + slice - 1) / slice) : 1u;
    if (plan.segments > n / 4) plan.segments = n / 4;
    if (env_segments) plan.segments = (u32)env_segments;
    if (plan.segments > n) plan.segments = n;
    if (plan.segments < 1) plan.segments = 1;
    const u32 per = (n + plan.segments - 1) / plan.segments;  // iterations per launch ...
    plan.segments = (n + per - 1) / per;                      // ... and the launches that makes
  }
  if (env_chunk) plan.chunk = (size_t)env_chunk;
  return plan;
}

// teams of blind_rotate_kernel<F, LOGN, K> the CURRENT device holds at once (occupancy x CUs), asked once per
// instantiation and device (a pool spans devices: nothing about one device is assumed of another)
template <class RK>
hipError_t resident_teams(unsigned* out) {
  static std::atomic<unsigned> cached[kMaxDevices];
  const int dev = current_device_slot();
  unsigned capacity = cached[dev].load(std::memory_order_acquire);
  if (capacity == 0) {
    auto kern = RK::get();
    int per_cu = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, RK::kThreads, RK::kLds);
    if (e != hipSuccess) return e;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    capacity = (unsigned)(per_cu > 0 ? per_cu : 1) * (unsigned)(cus > 0 ? cus : 256);
    cached[dev].store(capacity, std::memory_order_release);
  }
  *out = capacity;
  return hipSuccess;
}

// Which kernel rotates a batch of the PAIR shape (N = 512, k = 1, complex transform) that is too large for the wide team:
// one wave per sample takes ~2x the time of a two-wave team to finish ONE sample, and 2,048 of them fill the chip -- so up
// to what the chip holds as two-wave teams (1,536 samples) the team is faster (1,024 samples: 2.96 against 4.2 ms); above,
// the pair kernel's third fewer LDS cycles and 8 instead of 6 samples per CU win (4,096: 9.2 against 10.0 ms;
// profiles/r04_kernel_ab.txt).  TFHE_BR_PAIR_MIN overrides the threshold (batches >= it take the pair kernel).
template <class F, int LOGN, int K>
bool use_pair_kernel(size_t batch) {
  if constexpr (!pair_shape<F, LOGN, K>()) {
    return false;
  } else {
    static const long env_min = std::getenv("TFHE_BR_PAIR_MIN") ? std::atol(std::getenv("TFHE_BR_PAIR_MIN")) : -1;
    if (env_min >= 0) return batch >= (size_t)env_min;
    unsigned team_capacity = 0;
    if (resident_teams<RotateKernel<F, LOGN, K>>(&team_capacity) != hipSuccess) return true;
    return batch > (size_t)team_capacity * RotateKernel<F, LOGN, K>::kSamples;
  }
}

// The wide team (blind_rotate_wide_kernel) is offered for the complex transform up to N = 1024 while its row buffers fit
// the CU's LDS; it is USED for batches up to `wide_max_batch`: below that the chip has CUs to spare and a sample's latency
// -- not the chip's throughput -- is what a caller waits for (profiles/r04_batch_sweep*.txt).  TFHE_BR_WIDE overrides the
// threshold (0: never; n: batches up to n).
template <class F, int LOGN, int K>
constexpr bool wide_shape_ok() {
  return F::kLogShrink == 1 && F::kParts == 2 && LOGN <= 10 && field_shape_ok<F, LOGN>();
}
template <class F, int LOGN, int K>
size_t wide_max_batch(const PbsParams& P, int shape) {
  if constexpr (!wide_shape_ok<F, LOGN, K>()) {
    return 0;
  } else {
    using W = WideCfg<F, LOGN, K>;
    if (W::lds(P.levels) > (size_t)160 * 1024 || shape == launch::kShapeTeam) return 0;
    if (shape == launch::kShapeWide) return ~(size_t)0;
    static const long env_wide = std::getenv("TFHE_BR_WIDE") ? std::atol(std::getenv("TFHE_BR_WIDE")) : -1;
    if (env_wide >= 0) return (size_t)env_wide;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, current_device_slot()) != hipSuccess || cus <= 0) cus = 256;
    return (size_t)cus;  // one sample per CU
  }
}

template <class F, int LOGN, int K>
hipError_t launch_blind_rotate_wide(hipStream_t s, const PbsParams& P, const typename F::elem* tw, const u32* lwe_in, size_t batch,
                                    const u32* tv, size_t tv_stride, const typename F::elem* bsk, u32* glwe_out,
                                    u32* lwe_extracted) {
  if constexpr (!wide_shape_ok<F, LOGN, K>()) {
    return hipErrorInvalidValue;
  } else {
    using W = WideCfg<F, LOGN, K>;
    // the level counts with a key-ring instantiation (the BASELINE configurations' 2, 3, 6 and the full-word 4); any other
    // count runs the generic kernel
    auto launch = [&](auto levels_c) -> hipError_t {
      constexpr int LEVELS = decltype(levels_c)::value;
      auto kern = blind_rotate_wide_kernel<F, LOGN, K, LEVELS>;
      static std::atomic<unsigned long long> lds_done{0};
      hipError_t e = allow_lds(kern, (size_t)160 * 1024, lds_done);  // the size depends on the level count: allow the CU's whole LDS
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(W::kThreads), W::lds(P.levels), s, P, tw, lwe_in, batch, tv, tv_stride,
                         bsk, glwe_out, lwe_extracted, 0u, P.n, static_cast<u32*>(nullptr));
      return hipGetLastError();
    };
    switch (P.levels) {
      case 2: return launch(IntC<2>{});
      case 3: return launch(IntC<3>{});
      case 4: return launch(IntC<4>{});
      case 6: return launch(IntC<6>{});
      default: return launch(IntC<0>{});
    }
  }
}

// Multi-bit blind rotation (multibit.h): offered exactly where the wide team is.  0: offered; else launch::kMultibitNo*
template <class F, int LOGN, int K>
int multibit_refusal_of(const PbsParams& P) {
  if constexpr (F::kLogShrink != 1 || F::kParts != 2) {
    return launch::kMultibitNoBackend;
  } else if constexpr (!wide_shape_ok<F, LOGN, K>()) {
    return launch::kMultibitNoRing;
  } else {
    return WideCfg<F, LOGN, K>::lds(P.levels) > (size_t)160 * 1024 ? launch::kMultibitNoLds : 0;
  }
}

template <class F, int LOGN, int K>
hipError_t launch_multibit_bundle(hipStream_t s, const PbsParams& P, const void* tw_v, const u32* key, u32 g, const u32* lwe_in,
                                  size_t batch, void* bundles_v) {
  if constexpr (!wide_shape_ok<F, LOGN, K>()) {
    return hipErrorInvalidValue;
  } else {
    constexpr int N = 1 << LOGN;
    constexpr int waves = 4;  // polynomials per 256-thread workgroup
    const size_t lds = twiddle_bytes<F, LOGN>() + (size_t)N * 8 * waves;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto bundles = static_cast<typename F::elem*>(bundles_v);
    const u32 groups = multibit_groups(P.n, g);
    const u32 ggsw_polys = (K + 1) * P.levels * (K + 1);
    const size_t polys = (size_t)groups * ggsw_polys;
    if (polys > (size_t)0x7FFFFFFF || batch > 65535) return hipErrorInvalidValue;
    auto launch = [&](auto g_c) -> hipError_t {
      constexpr int GBITS = decltype(g_c)::value;
      auto kern = multibit_bundle_kernel<F, LOGN, GBITS>;
      static std::atomic<unsigned long long> lds_done{0};
      hipError_t e = allow_lds(kern, lds, lds_done);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, dim3((unsigned)((polys + waves - 1) / waves), (unsigned)batch), dim3(256), lds, s, tw, key, lwe_in, P.n,
                         groups, ggsw_polys, bundles, F::n_inv(LOGN - F::kLogShrink), key_layout_e<F, LOGN, K>());
      return hipGetLastError();
    };
    switch (g) {
      case 2: return launch(IntC<2>{});
      case 3: return launch(IntC<3>{});
      case 4: return launch(IntC<4>{});
      default: return hipErrorInvalidValue;
    }
  }
}

template <class F, int LOGN, int K>
hipError_t launch_multibit_rotate(hipStream_t s, const PbsParams& P, const void* tw_v, const u32* lwe_in, size_t batch, const u32* tv,
                                  size_t tv_stride, const void* bundles_v, u32 groups, u32* glwe_out, u32* lwe_extracted) {
  if constexpr (!wide_shape_ok<F, LOGN, K>()) {
    return hipErrorInvalidValue;
  } else {
    using W = WideCfg<F, LOGN, K>;
    if (W::lds(P.levels) > (size_t)160 * 1024) return hipErrorInvalidValue;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto bundles = static_cast<const typename F::elem*>(bundles_v);
    // the level counts with a key-ring instantiation, as launch_blind_rotate_wide picks them
    auto launch = [&](auto levels_c) -> hipError_t {
      constexpr int LEVELS = decltype(levels_c)::value;
      auto kern = multibit_rotate_wide_kernel<F, LOGN, K, LEVELS>;
      static std::atomic<unsigned long long> lds_done{0};
      hipError_t e = allow_lds(kern, (size_t)160 * 1024, lds_done);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(W::kThreads), W::lds(P.levels), s, P, tw, lwe_in, tv, tv_stride, bundles,
                         groups, glwe_out, lwe_extracted);
      return hipGetLastError();
    };
    switch (P.levels) {
      case 2: return launch(IntC<2>{});
      case 3: return launch(IntC<3>{});
      case 4: return launch(IntC<4>{});
      case 6: return launch(IntC<6>{});
      default: return launch(IntC<0>{});
    }
  }
}

template <class RK, class F, int LOGN, int K>
hipError_t plan_blind_rotate_with(const PbsParams& P, size_t batch, bool can_park, bool have_side, launch::BlindRotatePlanInfo* out, int shape) {
  {
    using C = TeamCfg<F, LOGN, K>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(RK::get(), RK::kLds, lds_done);
    unsigned capacity = 0;
    if (e == hipSuccess) e = resident_teams<RK>(&capacity);
    if (e != hipSuccess) return e;
    const size_t key_bytes = (size_t)P.n * (K + 1) * P.levels * (K + 1) * F::kParts * C::N * 8;
    const BlindRotatePlan plan = blind_rotate_plan<F>(batch, can_park, have_side, P.n, key_bytes, (u32)LOGN, (size_t)capacity * RK::kSamples);
    out->chunk = plan.chunk;
    out->segments = plan.segments;
    out->streams = plan.streams == 2 && plan.segments > 1 ? 2 : 1;
    out->resident_samples = (size_t)capacity * RK::kSamples;
    out->samples_per_team = RK::kSamples;
    out->waves_per_sample = RK::kWaves;
    if (batch > 0 && batch <= wide_max_batch<F, LOGN, K>(P, shape)) {  // the wide team: one launch over the whole key
      out->chunk = batch;
      out->segments = 1;
      out->streams = 1;
      out->samples_per_team = 1;
      out->waves_per_sample = 2 * (K + 1);
    }
    return hipSuccess;
  }
}

template <class F, int LOGN, int K>
hipError_t plan_blind_rotate(const PbsParams& P, size_t batch, bool can_park, bool have_side, launch::BlindRotatePlanInfo* out, int shape) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    if (use_pair_kernel<F, LOGN, K>(batch))
      return plan_blind_rotate_with<PairOrTeamKernel<F, LOGN, K>, F, LOGN, K>(P, batch, can_park, have_side, out, shape);
    return plan_blind_rotate_with<RotateKernel<F, LOGN, K>, F, LOGN, K>(P, batch, can_park, have_side, out, shape);
  }
}

template <class RK, class F, int LOGN, int K>
hipError_t launch_blind_rotate_with(hipStream_t s, const PbsParams& P, const typename F::elem* tw, const u32* lwe_in,
                                    size_t batch, const u32* tv, size_t tv_stride, const typename F::elem* bsk,
                                    u32* glwe_out, u32* lwe_extracted, u32* state, const launch::SideStream* side) {
  {
    using C = TeamCfg<F, LOGN, K>;
    auto kern = RK::get();
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, RK::kLds, lds_done);
    if (e != hipSuccess) return e;
    unsigned capacity = 0;
    if ((e = resident_teams<RK>(&capacity)) != hipSuccess) return e;
    // a second stream cannot be forked inside a stream capture that the caller ends on `s` alone without it joining;
    // it does join (below), but a capture is no place for a measured policy: one stream there
    bool have_side = side && side->stream && side->fork && side->join;
    if (have_side) {
      hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(s, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) have_side = false;
    }
    const size_t key_bytes = (size_t)P.n * (K + 1) * P.levels * (K + 1) * F::kParts * C::N * 8;
    const BlindRotatePlan plan =
        blind_rotate_plan<F>(batch, state != nullptr, have_side, P.n, key_bytes, (u32)LOGN, (size_t)capacity * RK::kSamples);
    const int parts = plan.streams == 2 && plan.segments > 1 ? 2 : 1;
    const u32 per = (P.n + plan.segments - 1) / plan.segments;
    if (parts == 2) {  // fork: the side stream starts after everything already on s
      if ((e = hipEventRecord(side->fork, s)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(side->stream, side->fork, 0)) != hipSuccess) return e;
    }
    for (size_t off = 0; off < batch; off += plan.chunk) {
      const size_t here = batch - off < plan.chunk ? batch - off : plan.chunk;
      // part q = samples [q * share, (q + 1) * share) of the chunk; share is a multiple of the samples per team
      const size_t share = (((here + parts - 1) / parts + RK::kSamples - 1) / RK::kSamples) * RK::kSamples;
      for (u32 i0 = 0; i0 < P.n; i0 += per) {
        const u32 i1 = i0 + per < P.n ? i0 + per : P.n;
        for (int q = 0; q < parts; ++q) {
          if ((size_t)q * share >= here) break;
          const size_t o = off + (size_t)q * share;
          const size_t cnt = here - (size_t)q * share < share ? here - (size_t)q * share : share;
          hipLaunchKernelGGL(kern, dim3((unsigned)((cnt + RK::kSamples - 1) / RK::kSamples)), dim3(RK::kThreads), RK::kLds,
                             q ? side->stream : s, P, tw, lwe_in + o * ((size_t)P.n + 1), cnt, tv + o * tv_stride,
                             tv_stride, bsk, glwe_out ? glwe_out + o * (size_t)(K + 1) * C::N : nullptr,
                             lwe_extracted ? lwe_extracted + o * ((size_t)K * C::N + 1) : nullptr, i0, i1,
                             state ? state + o * (size_t)(K + 1) * C::N : nullptr);
          e = hipGetLastError();
          if (e != hipSuccess) return e;
        }
      }
    }
    if (parts == 2) {  // join: whatever follows on s waits for the side stream
      if ((e = hipEventRecord(side->join, side->stream)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(s, side->join, 0)) != hipSuccess) return e;
    }
    return hipSuccess;
  }
}

template <class F, int LOGN, int K>
hipError_t launch_blind_rotate(hipStream_t s, const PbsParams& P, const void* tw_v, const u32* lwe_in,
                               size_t batch, const u32* tv, size_t tv_stride, const void* bsk_v,
                               u32* glwe_out, u32* lwe_extracted, u32* state, const launch::SideStream* side, int shape) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;  // the context never picks such a field (capi.cpp)
  } else {
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto bsk = static_cast<const typename F::elem*>(bsk_v);
    if constexpr (wide_shape_ok<F, LOGN, K>()) {
      if (batch <= wide_max_batch<F, LOGN, K>(P, shape))
        return launch_blind_rotate_wide<F, LOGN, K>(s, P, tw, lwe_in, batch, tv, tv_stride, bsk, glwe_out, lwe_extracted);
    }
    if (use_pair_kernel<F, LOGN, K>(batch))
      return launch_blind_rotate_with<PairOrTeamKernel<F, LOGN, K>, F, LOGN, K>(s, P, tw, lwe_in, batch, tv, tv_stride, bsk, glwe_out,
                                                                               lwe_extracted, state, side);
    return launch_blind_rotate_with<RotateKernel<F, LOGN, K>, F, LOGN, K>(s, P, tw, lwe_in, batch, tv, tv_stride, bsk, glwe_out,
                                                                          lwe_extracted, state, side);
  }
}

// Block-binary blind rotation (block_rotate.h): the complex transform with one wave per polynomial, N = 512 and 1024
template <class F, int LOGN, int K>
constexpr bool block_shape_ok() {
  return F::kLogShrink == 1 && F::kParts == 2 && LOGN >= 9 && LOGN <= 10;
}
template <class F, int LOGN, int K>
struct BlockRotateKernel {
  using C = TeamCfg<F, LOGN, K, 1>;
  static constexpr int kThreads = C::kThreads;
  static constexpr size_t kLds = C::kLds;
  static constexpr int kSamples = 1;
  static constexpr int kWaves = C::kWaves;
  static auto get() { return block_rotate_kernel<F, LOGN, K>; }
};

// launch_blind_rotate_with's walk -- blind_rotate_plan unchanged, chunks, segments, two streams -- with every segment's
// length rounded up to a multiple of `block`, so that a launch starts on a block boundary
template <class F, int LOGN, int K>
hipError_t launch_block_rotate(hipStream_t s, const PbsParams& P, const void* tw_v, const void* roots_v, const u32* lwe_in, size_t batch,
                               const u32* tv, size_t tv_stride, const void* bsk_v, u32 block, u32* glwe_out, u32* lwe_extracted,
                               u32* state, const launch::SideStream* side) {
  if constexpr (!block_shape_ok<F, LOGN, K>()) {
    return hipErrorInvalidValue;
  } else {
    using RK = BlockRotateKernel<F, LOGN, K>;
    using C = typename RK::C;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto roots = static_cast<const typename F::elem*>(roots_v);
    auto bsk = static_cast<const typename F::elem*>(bsk_v);
    auto kern = RK::get();
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, RK::kLds, lds_done);
    if (e != hipSuccess) return e;
    unsigned capacity = 0;
    if ((e = resident_teams<RK>(&capacity)) != hipSuccess) return e;
    bool have_side = side && side->stream && side->fork && side->join;
    if (have_side) {  // one stream inside a capture, as launch_blind_rotate_with
      hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(s, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) have_side = false;
    }
    const size_t key_bytes = (size_t)P.n * (K + 1) * P.levels * (K + 1) * F::kParts * C::N * 8;
    const BlindRotatePlan plan = blind_rotate_plan<F>(batch, state != nullptr, have_side, P.n, key_bytes, (u32)LOGN, (size_t)capacity);
    u32 per = (P.n + plan.segments - 1) / plan.segments;
    per = (per + block - 1) / block * block;
    const int parts = plan.streams == 2 && per < P.n ? 2 : 1;
    if (parts == 2) {
      if ((e = hipEventRecord(side->fork, s)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(side->stream, side->fork, 0)) != hipSuccess) return e;
    }
    for (size_t off = 0; off < batch; off += plan.chunk) {
      const size_t here = batch - off < plan.chunk ? batch - off : plan.chunk;
      const size_t share = (here + parts - 1) / parts;
      for (u32 i0 = 0; i0 < P.n; i0 += per) {
        const u32 i1 = P.n - i0 > per ? i0 + per : P.n;
        for (int q = 0; q < parts; ++q) {
          if ((size_t)q * share >= here) break;
          const size_t o = off + (size_t)q * share;
          const size_t cnt = here - (size_t)q * share < share ? here - (size_t)q * share : share;
          hipLaunchKernelGGL(kern, dim3((unsigned)cnt), dim3(RK::kThreads), RK::kLds, q ? side->stream : s, P, tw, roots,
                             lwe_in + o * ((size_t)P.n + 1), tv + o * tv_stride, tv_stride, bsk, block,
                             glwe_out ? glwe_out + o * (size_t)(K + 1) * C::N : nullptr,
                             lwe_extracted ? lwe_extracted + o * ((size_t)K * C::N + 1) : nullptr, i0, i1,
                             state ? state + o * (size_t)(K + 1) * C::N : nullptr);
          e = hipGetLastError();
          if (e != hipSuccess) return e;
        }
      }
    }
    if (parts == 2) {
      if ((e = hipEventRecord(side->join, side->stream)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(s, side->join, 0)) != hipSuccess) return e;
    }
    return hipSuccess;
  }
}

template <class F, int LOGN, int K>
hipError_t launch_blind_rotate_bmmp(hipStream_t s, const PbsParams& P, const void* tw_v, const u32* lwe_in,
                                    size_t batch, const u32* tv, size_t tv_stride, const void* bsk_v,
                                    u32* glwe_out, u32* lwe_extracted) {
  // (the unrolled rotation in the complex transform was measured and is not offered: profiles/r04_kernel_ab.txt)
  if constexpr (LOGN != 9 || !(F::kId == GlField::kId || F::kId == Fp49Field::kId)) {
    return hipErrorInvalidValue;  // shape_supported_bmmp() / field_supported_bmmp() keep callers away
  } else {
    using C = TeamCfg<F, LOGN, K, 1>;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto bsk = static_cast<const typename F::elem*>(bsk_v);
    auto kern = blind_rotate_bmmp_kernel<F, LOGN, K>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, C::kLds, lds_done);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(C::kThreads), C::kLds, s, P, tw, lwe_in, batch,
                       tv, tv_stride, bsk, glwe_out, lwe_extracted);
    return hipGetLastError();
  }
}

template <class F, int LOGN, int K>
hipError_t launch_external_product(hipStream_t s, const PbsParams& P, const void* tw_v,
                                   const void* ggsw_v, size_t ggsw_stride_words, const u32* glwe_in,
                                   u32* ct1_inout, const u32* cmux_ct0, size_t batch, u32* glwe_out,
                                   unsigned long long* queue) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    using C = TeamCfg<F, LOGN, K, 1>;
    constexpr size_t kLdsWithTicket = C::kLds + 16;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto ggsw = static_cast<const typename F::elem*>(ggsw_v);
    auto kern = external_product_kernel<F, LOGN, K>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, kLdsWithTicket, lds_done);
    if (e != hipSuccess) return e;
    // persistent grid: as many teams as the device keeps resident at once (LDS or registers decide)
    static std::atomic<int> resident_per_device[kMaxDevices];
    const int dev_slot = current_device_slot();
    std::atomic<int>& resident = resident_per_device[dev_slot];
    int teams = resident.load(std::memory_order_relaxed);
    if (teams == 0) {
      int dev = dev_slot, cus = 0, per_cu = 0;
      e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
      if (e == hipSuccess)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), C::kThreads, kLdsWithTicket);
      if (e != hipSuccess) return e;
      teams = cus * (per_cu > 0 ? per_cu : 1);
      resident.store(teams, std::memory_order_relaxed);
    }
    const size_t grid = batch < (size_t)teams ? batch : (size_t)teams;
    // the work queue pays from 16 samples per team (see the kernel)
    unsigned long long* use_queue = batch / grid >= 16 ? queue : nullptr;
    if (use_queue && (e = hipMemsetAsync(use_queue, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    // the stride arrives in 8-byte words; the kernel counts elements
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(C::kThreads), kLdsWithTicket, s, P, tw, ggsw,
                       ggsw_stride_words / (sizeof(typename F::elem) / 8), glwe_in, ct1_inout, cmux_ct0, batch, glwe_out, use_queue);
    return hipGetLastError();
  }
}

// workgroups a packing launch aims at: the slices of an output are cut into runs until the grid reaches a few teams
// per team slot of the chip (1,024 at cfg2); more runs mean more partial results to add atomically
constexpr unsigned kPackTargetWgs = 2048u;

template <class F, int LOGN, int K>
hipError_t launch_pack_lwe(hipStream_t s, const PbsParams& P, const void* tw_v, const void* key_v, const u32* cols,
                           u32 d, size_t groups, u32* glwe_out) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    using C = TeamCfg<F, LOGN, K, 1>;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto key = static_cast<const typename F::elem*>(key_v);
    auto kern = pack_lwe_kernel<F, LOGN, K>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, C::kLds, lds_done);
    if (e != hipSuccess) return e;
    const u32 slices = (d + K) / (K + 1);
    size_t runs = kPackTargetWgs / groups;
    if (runs > slices) runs = slices;
    if (runs > 65535u) runs = 65535u;
    if (runs < 1u) runs = 1u;
    const u32 per_run = (u32)((slices + runs - 1) / runs);
    runs = (slices + per_run - 1) / per_run;
    hipLaunchKernelGGL(kern, dim3((unsigned)groups, (unsigned)runs), dim3(C::kThreads), C::kLds, s, P, tw, key, cols, d,
                       slices, per_run, glwe_out);
    return hipGetLastError();
  }
}

template <class F, int LOGN, int K>
hipError_t launch_glwe_switch(hipStream_t s, const PbsParams& P, const void* tw_v, const void* key_v, const u32* glwe_in,
                              size_t batch, u32 t_inv, bool add_input, u32* glwe_out) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    using C = TeamCfg<F, LOGN, K, 1>;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto key = static_cast<const typename F::elem*>(key_v);
    auto kern = glwe_switch_kernel<F, LOGN, K>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, C::kLds, lds_done);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(C::kThreads), C::kLds, s, P, tw, key, glwe_in, t_inv,
                       add_input ? 1u : 0u, glwe_out);
    return hipGetLastError();
  }
}

// The three pass kernels -- cmux_tree_kernel, demux_tree_kernel, cmux_program_kernel -- share a team (TeamCfg<.., 1>)
// and a signature (P, the twiddles, the pass struct by value): one trait, the kernel named by its pass struct.  Which
// passes go out, with how many teams and over which workspace, is host arithmetic (passes.h; capi.cpp sequences them).
template <class F, int LOGN, int K, class Pass>
struct PassKernel {
  using C = TeamCfg<F, LOGN, K, 1>;
  static constexpr int kThreads = C::kThreads;
  static constexpr size_t kLds = C::kLds;
  static auto get() {
    if constexpr (std::is_same<Pass, CmuxTreePass>::value) return cmux_tree_kernel<F, LOGN, K>;
    else if constexpr (std::is_same<Pass, DemuxTreePass>::value) return demux_tree_kernel<F, LOGN, K>;
    else return cmux_program_kernel<F, LOGN, K>;
  }
};

template <class F, int LOGN, int K, class Pass>
hipError_t pass_resident_teams(unsigned* out) {
  if constexpr (!field_shape_ok<F, LOGN>()) return hipErrorInvalidValue;
  else return resident_teams<PassKernel<F, LOGN, K, Pass>>(out);
}

// pass.query_stride arrives in 8-byte words, like launch_external_product's stride.  One instantiation per kernel, so
// one lds_done flag per kernel.
template <class F, int LOGN, int K, class Pass>
hipError_t launch_pass(hipStream_t s, const PbsParams& P, const void* tw_v, Pass pass, size_t teams) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    using PK = PassKernel<F, LOGN, K, Pass>;
    if (teams == 0 || teams > kMaxGrid) return hipErrorInvalidValue;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto kern = PK::get();
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, PK::kLds, lds_done);
    if (e != hipSuccess) return e;
    pass.query_stride /= sizeof(typename F::elem) / 8;
    hipLaunchKernelGGL(kern, dim3((unsigned)teams), dim3(PK::kThreads), PK::kLds, s, P, tw, pass);
    return hipGetLastError();
  }
}

template <class F, int LOGN>
hipError_t launch_bsk_prepare(hipStream_t s, const void* tw_v, const u32* polys, size_t poly_count,
                              void* spectra_v, u32 k) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    constexpr int N = 1 << LOGN;
    constexpr int G = GroupOf<F, LOGN>::value;
    constexpr int groups = 4 / G;  // polynomials per 256-thread workgroup
    const size_t lds = twiddle_bytes<F, LOGN>() + (size_t)N * 8 * groups;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto spectra = static_cast<typename F::elem*>(spectra_v);
    auto kern = bsk_prepare_kernel<F, LOGN>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, lds, lds_done);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((poly_count + groups - 1) / groups);
    const int layout_e = k == 1 ? key_layout_e<F, LOGN, 1>() : k == 2 ? key_layout_e<F, LOGN, 2>() : 0;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, tw, polys, poly_count, spectra,
                       F::n_inv(LOGN - F::kLogShrink), layout_e);
    return hipGetLastError();
  }
}

template <class F, int LOGN>
hipError_t launch_conv_weights(hipStream_t s, const void* tw_v, const i32* polys, size_t poly_count, void* spectra_v) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    constexpr int N = 1 << LOGN;
    constexpr int G = GroupOf<F, LOGN>::value;
    constexpr int groups = 4 / G;  // polynomials per 256-thread workgroup
    const size_t lds = twiddle_bytes<F, LOGN>() + (size_t)N * 8 * groups;
    auto kern = conv_weights_kernel<F, LOGN>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, lds, lds_done);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((poly_count + groups - 1) / groups);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, static_cast<const typename F::elem*>(tw_v), polys, poly_count,
                       static_cast<typename F::elem*>(spectra_v));
    return hipGetLastError();
  }
}

template <class F, int LOGN, int K>
hipError_t launch_glwe_conv(hipStream_t s, const void* tw_v, const GlweConvArgs& args, size_t queries) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    using C = TeamCfg<F, LOGN, K, 1>;
    auto kern = glwe_conv_kernel<F, LOGN, K>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, C::kLds, lds_done);
    if (e != hipSuccess) return e;
    const size_t teams = queries * args.outputs;
    if (teams == 0 || teams > kMaxGrid || args.rows_per_pass == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)teams), dim3(C::kThreads), C::kLds, s, static_cast<const typename F::elem*>(tw_v), args);
    return hipGetLastError();
  }
}

template <class F, int LOGN>
hipError_t launch_glwe_body(hipStream_t s, const void* tw_v, u32 k, const u32* rows, size_t row_count,
                            const u32* sk, u32* dst, size_t dst_stride, u32 negate) {
  if constexpr (!field_shape_ok<F, LOGN>()) {
    return hipErrorInvalidValue;
  } else {
    constexpr int N = 1 << LOGN;
    constexpr int G = GroupOf<F, LOGN>::value;
    constexpr int groups = 4 / G;  // rows per 256-thread workgroup
    const size_t lds = twiddle_bytes<F, LOGN>() + (size_t)N * 8 * groups;
    auto tw = static_cast<const typename F::elem*>(tw_v);
    auto kern = glwe_body_kernel<F, LOGN>;
    static std::atomic<unsigned long long> lds_done{0};
    hipError_t e = allow_lds(kern, lds, lds_done);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((row_count + groups - 1) / groups);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, tw, k, rows, row_count, sk, dst, dst_stride,
                       negate, F::n_inv(LOGN - F::kLogShrink));
    return hipGetLastError();
  }
}

}  // namespace

namespace launch {

bool shape_supported(u32 log_n, u32 k) { return log_n >= 9 && log_n <= 11 && (k == 1 || k == 2); }

bool shape_supported_bmmp(u32 log_n, u32 k) { return log_n == 9 && (k == 1 || k == 2); }

// The unrolled blind rotation carries three accumulator sets per wave.  Offered where that fits the registers and the
// mode is at least even with the loop: Goldilocks (+10 % at the reference's default parameters) and the single-spectrum
// 49-bit field (-5 %, 17-23 spilled registers).  In the two-spectra fields it ran 1.9-3.4x slower than the loop on 50-172
// spilled registers (profiles/r02_kernel_ab.txt, r02_h_isa_resources_all_kernels.txt): not instantiated, refused at load.
bool field_supported_bmmp(int field) { return field == kFieldGoldilocks || field == kFieldFp49; }

int field_parts(int field) { return (field == kFieldGoldilocks || field == kFieldFp49) ? 1 : 2; }

bool field_shape_supported(int field, u32 log_n) {
  return field != kFieldFft || (log_n >= 9 && log_n <= 11);
}

int samples_per_team(int field, u32 log_n, u32 k) {
  if (field != kFieldFft) return 1;
  if (log_n == 11) return k == 2 ? SamplesPerTeam<FftField, 11, 2>::value : SamplesPerTeam<FftField, 11, 1>::value;
  if (log_n == 9) return k == 2 ? SamplesPerTeam<FftField, 9, 2>::value : SamplesPerTeam<FftField, 9, 1>::value;
  return 1;
}

// (field, log_n, k) -> template instantiation.  TFHE_DEV_CFG2_ONLY builds just the BASELINE cfg2
// shape (N = 1024, k = 1) for fast iteration on the kernels.
#if defined(TFHE_DEV_CFG2_ONLY)
#ifndef TFHE_DEV_LOGN
#define TFHE_DEV_LOGN 10
#define TFHE_DEV_K 1
#endif
#define TFHE_DISPATCH_LOGN_K(log_n, k, CALL)                                  \
  if ((k) == TFHE_DEV_K && (log_n) == TFHE_DEV_LOGN) {                        \
    constexpr int KK = TFHE_DEV_K;                                            \
    constexpr int LL = TFHE_DEV_LOGN;                                         \
    return CALL;                                                              \
  }
#define TFHE_DISPATCH_LOGN(log_n, CALL)                                       \
  if ((log_n) == TFHE_DEV_LOGN) {                                             \
    constexpr int LL = TFHE_DEV_LOGN;                                         \
    return CALL;                                                              \
  }
#else
#define TFHE_DISPATCH_LOGN_K(log_n, k, CALL)                                  \
  if ((k) == 1) {                                                             \
    constexpr int KK = 1;                                                     \
    switch (log_n) {                                                          \
      case 9: { constexpr int LL = 9; return CALL; }                          \
      case 10: { constexpr int LL = 10; return CALL; }                        \
      case 11: { constexpr int LL = 11; return CALL; }                        \
      default: break;                                                         \
    }                                                                         \
  } else if ((k) == 2) {                                                      \
    constexpr int KK = 2;                                                     \
    switch (log_n) {                                                          \
      case 9: { constexpr int LL = 9; return CALL; }                          \
      case 10: { constexpr int LL = 10; return CALL; }                        \
      case 11: { constexpr int LL = 11; return CALL; }                        \
      default: break;                                                         \
    }                                                                         \
  }
#define TFHE_DISPATCH_LOGN(log_n, CALL)                                       \
  switch (log_n) {                                                            \
    case 9: { constexpr int LL = 9; return CALL; }                            \
    case 10: { constexpr int LL = 10; return CALL; }                          \
    case 11: { constexpr int LL = 11; return CALL; }                          \
    default: break;                                                           \
  }
#endif

#if defined(TFHE_DEV_FIELD_FP_ONLY) || defined(TFHE_DEV_FIELD_FP49_ONLY) || defined(TFHE_DEV_FIELD_FFT_ONLY)  // dev builds: one field (fast iteration)
#if defined(TFHE_DEV_FIELD_FP49_ONLY)
#define TFHE_DEV_FIELD_ID kFieldFp49
#define TFHE_DEV_FIELD_T Fp49Field
#elif defined(TFHE_DEV_FIELD_FFT_ONLY)
#define TFHE_DEV_FIELD_ID kFieldFft
#define TFHE_DEV_FIELD_T FftField
#else
#define TFHE_DEV_FIELD_ID kFieldFp64
#define TFHE_DEV_FIELD_T FpField
#endif
#define TFHE_DISPATCH_FIELD(field, BODY)                                      \
  do {                                                                        \
    if ((field) == TFHE_DEV_FIELD_ID) {                                       \
      typedef TFHE_DEV_FIELD_T FF;                                            \
      BODY                                                                    \
    }                                                                         \
    return hipErrorInvalidValue;                                              \
  } while (0)
#else
#define TFHE_DISPATCH_FIELD(field, BODY)                                      \
  do {                                                                        \
    if ((field) == kFieldGoldilocks) {                                        \
      typedef GlField FF;                                                     \
      BODY                                                                    \
    } else if ((field) == kFieldFp64) {                                       \
      typedef FpField FF;                                                     \
      BODY                                                                    \
    } else if ((field) == kFieldGoldilocksSplit) {                            \
      typedef GlSplitField FF;                                                \
      BODY                                                                    \
    } else if ((field) == kFieldFp49) {                                       \
      typedef Fp49Field FF;                                                   \
      BODY                                                                    \
    } else if ((field) == kFieldFft) {                                        \
      typedef FftField FF;                                                    \
      BODY                                                                    \
    }                                                                         \
    return hipErrorInvalidValue;                                              \
  } while (0)
#endif

hipError_t bsk_prepare(hipStream_t s, int field, u32 log_n, u32 k, const void* tw, const u32* polys,
                       size_t poly_count, void* spectra) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN(log_n, (launch_bsk_prepare<FF, LL>(s, tw, polys, poly_count, spectra, k))));
}

hipError_t multibit_refusal(int field, const PbsParams& P, int* why) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (*why = multibit_refusal_of<FF, LL, KK>(P), hipSuccess)));
}

hipError_t multibit_bundle(hipStream_t s, int field, const PbsParams& P, const void* tw, const u32* key, u32 g, const u32* lwe_in,
                           size_t batch, void* bundles) {
  if (batch == 0) return hipErrorInvalidValue;
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_multibit_bundle<FF, LL, KK>(s, P, tw, key, g, lwe_in, batch, bundles))));
}

hipError_t multibit_rotate(hipStream_t s, int field, const PbsParams& P, const void* tw, const u32* lwe_in, size_t batch, const u32* tv,
                           size_t tv_stride, const void* bundles, u32 groups, u32* glwe_out, u32* lwe_extracted) {
  if (batch == 0 || batch > 0x7FFFFFFFull || groups == 0) return hipErrorInvalidValue;
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_multibit_rotate<FF, LL, KK>(s, P, tw, lwe_in, batch, tv, tv_stride,
                                                                                                 bundles, groups, glwe_out, lwe_extracted))));
}

bool block_rotate_supported(int field, u32 log_n, u32 k) {
  return field == kFieldFft && (log_n == 9 || log_n == 10) && (k == 1 || k == 2);
}

hipError_t block_rotate(hipStream_t s, int field, const PbsParams& P, const void* tw, const void* roots, const u32* lwe_in, size_t batch,
                        const u32* tv, size_t tv_stride, const void* bsk, u32 block, u32* glwe_out, u32* lwe_extracted, u32* state,
                        const SideStream* side) {
  if (batch == 0 || block < 2 || !block_rotate_supported(field, P.log_n, P.k)) return hipErrorInvalidValue;
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_block_rotate<FF, LL, KK>(s, P, tw, roots, lwe_in, batch, tv, tv_stride, bsk,
                                                                                              block, glwe_out, lwe_extracted, state, side))));
}

hipError_t blind_rotate(hipStream_t s, int field, const PbsParams& P, const void* tw,
                        const u32* lwe_in, size_t batch, const u32* tv, size_t tv_stride,
                        const void* bsk, u32* glwe_out, u32* lwe_extracted, u32* state, const SideStream* side, int shape) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k,
                      (launch_blind_rotate<FF, LL, KK>(s, P, tw, lwe_in, batch, tv, tv_stride, bsk,
                                                       glwe_out, lwe_extracted, state, side, shape))));
}

hipError_t blind_rotate_plan(int field, const PbsParams& P, size_t batch, bool can_park, bool have_side,
                             BlindRotatePlanInfo* out, int shape) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (plan_blind_rotate<FF, LL, KK>(P, batch, can_park, have_side, out, shape))));
}

hipError_t blind_rotate_bmmp(hipStream_t s, int field, const PbsParams& P, const void* tw,
                             const u32* lwe_in, size_t batch, const u32* tv, size_t tv_stride,
                             const void* bsk, u32* glwe_out, u32* lwe_extracted) {
  if (!shape_supported_bmmp(P.log_n, P.k) || (P.n & 1u)) return hipErrorInvalidValue;
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k,
                      (launch_blind_rotate_bmmp<FF, LL, KK>(s, P, tw, lwe_in, batch, tv, tv_stride, bsk,
                                                            glwe_out, lwe_extracted))));
}

hipError_t external_product(hipStream_t s, int field, const PbsParams& P, const void* tw,
                            const void* ggsw, size_t ggsw_stride_words, const u32* glwe_in,
                            u32* ct1_inout, const u32* cmux_ct0, size_t batch, u32* glwe_out,
                            unsigned long long* queue) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k,
                      (launch_external_product<FF, LL, KK>(s, P, tw, ggsw, ggsw_stride_words, glwe_in,
                                                           ct1_inout, cmux_ct0, batch, glwe_out, queue))));
}

hipError_t pack_transpose(hipStream_t s, const u32* lwe_in, size_t groups, u32 per_group, u32 d, u32 log_n, u32* cols,
                          u32 log_rep) {
  const unsigned gz = (unsigned)(groups < 65535u ? groups : 65535u);
  dim3 grid((d + 1 + kPackTile - 1) / kPackTile, (1u << log_n) / kPackTile, gz);
  hipLaunchKernelGGL(pack_transpose_kernel, grid, dim3(256), 0, s, lwe_in, groups, per_group, d, log_n, cols, log_rep);
  return hipGetLastError();
}

hipError_t tree_lut_expand(hipStream_t s, const u32* in, size_t count, size_t per_row, u32 words, u32* out) {
  const unsigned grid = (unsigned)(count < ((size_t)1 << 20) ? count : (size_t)1 << 20);
  hipLaunchKernelGGL(tree_lut_expand_kernel, dim3(grid), dim3(256), 0, s, in, count, per_row, words, out);
  return hipGetLastError();
}

hipError_t tree_lut_test_vectors(hipStream_t s, const u32* table, size_t set_stride, size_t count, size_t per_row, u32 log_p,
                                 u32 log_n, u32* tv) {
  const unsigned grid = (unsigned)(count < ((size_t)1 << 20) ? count : (size_t)1 << 20);
  hipLaunchKernelGGL(tree_lut_test_vectors_kernel, dim3(grid), dim3(256), 0, s, table, set_stride, count, per_row, log_p, log_n, tv);
  return hipGetLastError();
}

hipError_t pack_lwe(hipStream_t s, int field, const PbsParams& P, const void* tw, const void* key, const u32* cols, u32 d,
                    size_t groups, u32* glwe_out) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_pack_lwe<FF, LL, KK>(s, P, tw, key, cols, d, groups, glwe_out))));
}

hipError_t packing_add_gadget(hipStream_t s, u32* pksk, size_t rows, u32 k, u32 log_n, const u32* factor) {
  hipLaunchKernelGGL(packing_add_gadget_kernel, dim3(grid_for(rows, 256)), dim3(256), 0, s, pksk, rows, k, log_n, factor);
  return hipGetLastError();
}

hipError_t glwe_switch(hipStream_t s, int field, const PbsParams& P, const void* tw, const void* key, const u32* glwe_in,
                       size_t batch, u32 t_inv, bool add_input, u32* glwe_out) {
  if (batch == 0 || batch > 0x7FFFFFFFull || !(t_inv & 1u) || t_inv >= (2u << P.log_n)) return hipErrorInvalidValue;
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_glwe_switch<FF, LL, KK>(s, P, tw, key, glwe_in, batch, t_inv,
                                                                                              add_input, glwe_out))));
}

hipError_t glwe_automorphism(hipStream_t s, const u32* glwe_in, size_t polys, u32 log_n, u32 t_inv, u32* glwe_out) {
  if (polys == 0 || log_n > 14 || !(t_inv & 1u) || t_inv >= (2u << log_n)) return hipErrorInvalidValue;  // N words of LDS
  const unsigned grid = (unsigned)(polys < ((size_t)1 << 20) ? polys : (size_t)1 << 20);
  hipLaunchKernelGGL(glwe_automorphism_kernel, dim3(grid), dim3(256), sizeof(u32) << log_n, s, glwe_in, polys, log_n, t_inv, glwe_out);
  return hipGetLastError();
}

hipError_t glwe_switch_add_gadget(hipStream_t s, u32* key, u32 k, u32 log_n, u32 levels, u32 log_base, u32 top,
                                  const i32* from_polys) {
  const size_t total = ((size_t)k * levels) << log_n;
  hipLaunchKernelGGL(glwe_switch_add_gadget_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, key, k, log_n, levels, log_base, top,
                     from_polys);
  return hipGetLastError();
}

hipError_t tree_resident_teams(int field, const PbsParams& P, unsigned* out) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (pass_resident_teams<FF, LL, KK, CmuxTreePass>(out))));
}

hipError_t cmux_tree_pass(hipStream_t s, int field, const PbsParams& P, const void* tw, const CmuxTreePass& pass, size_t teams) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_pass<FF, LL, KK>(s, P, tw, pass, teams))));
}

hipError_t demux_resident_teams(int field, const PbsParams& P, unsigned* out) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (pass_resident_teams<FF, LL, KK, DemuxTreePass>(out))));
}

hipError_t demux_tree_pass(hipStream_t s, int field, const PbsParams& P, const void* tw, const DemuxTreePass& pass, size_t teams) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_pass<FF, LL, KK>(s, P, tw, pass, teams))));
}

hipError_t program_resident_teams(int field, const PbsParams& P, unsigned* out) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (pass_resident_teams<FF, LL, KK, CmuxProgramPass>(out))));
}

hipError_t cmux_program_pass(hipStream_t s, int field, const PbsParams& P, const void* tw, const CmuxProgramPass& pass, size_t queries) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(P.log_n, P.k, (launch_pass<FF, LL, KK>(s, P, tw, pass, queries * pass.parts))));
}

hipError_t key_switch_plan(const KsParams& K, u32 big_n, u32 n, size_t batch, int path, KeySwitchPlanInfo* out) {
  if (batch == 0 || !out) return hipErrorInvalidValue;
  const bool admitted = ksm_admitted(K.log_base, K.levels, big_n);
  if (path == kKsPathMatrix && !admitted) return hipErrorInvalidValue;
  out->matrix = path == kKsPathMatrix || (path == kKsPathAuto && admitted && batch >= kKsMatrixMinBatch);
  if (out->matrix) {
    const KsmLayout lo = ksm_layout(big_n, K.levels, n);
    out->grid_x = lo.col_tiles / kKsmColTiles;
    out->grid_y = (unsigned)((batch + 4 * kKsmSamples - 1) / (4 * kKsmSamples));
    // aim at kKsmTargetWgs workgroups; a split covers whole super-blocks
    unsigned splits = kKsmTargetWgs / (out->grid_x * out->grid_y);
    if (splits > lo.sblocks) splits = lo.sblocks;
    if (splits < 1u) splits = 1u;
    out->per_split = (lo.sblocks + splits - 1) / splits;
    out->splits = (lo.sblocks + out->per_split - 1) / out->per_split;
    return hipSuccess;
  }
  out->grid_x = (n + 1 + kKsCols - 1) / kKsCols;
  out->grid_y = (unsigned)((batch + kKsSamples - 1) / kKsSamples);
  // aim at kKsTargetWgs workgroups; a split covers a multiple of kKsWords words, at least 64
  unsigned splits = kKsTargetWgs / (out->grid_x * out->grid_y);
  const unsigned max_splits = (big_n + 63u) / 64u;
  if (splits > max_splits) splits = max_splits;
  if (splits > 32u) splits = 32u;
  if (splits < 1u) splits = 1u;
  out->per_split = ((big_n + splits - 1) / splits + kKsWords - 1) / kKsWords * kKsWords;
  out->splits = (big_n + out->per_split - 1) / out->per_split;
  return hipSuccess;
}

size_t ksk_matrix_bytes(const KsParams& K, u32 big_n, u32 n) { return ksm_bytes(ksm_layout(big_n, K.levels, n)); }

hipError_t ksk_prepare_matrix(hipStream_t s, const KsParams& K, u32 big_n, u32 n, const u32* ksk, void* prepared) {
  const KsmLayout lo = ksm_layout(big_n, K.levels, n);
  const size_t threads = (size_t)lo.sblocks * lo.levels * lo.col_tiles * 64;
  hipLaunchKernelGGL(ksk_prepare_matrix_kernel, dim3(grid_for(threads, 256)), dim3(256), 0, s, lo, ksk,
                     static_cast<unsigned char*>(prepared));
  return hipGetLastError();
}

hipError_t key_switch(hipStream_t s, const KsParams& K, u32 big_n, u32 n, const u32* lwe_in,
                      size_t batch, const u32* ksk, u32* lwe_out, const void* ksk_matrix, int path) {
  KeySwitchPlanInfo plan{};
  hipError_t e = key_switch_plan(K, big_n, n, batch, path, &plan);
  if (e != hipSuccess) return e;
  if (plan.matrix && !ksk_matrix) return hipErrorInvalidValue;  // a missing prepared key is an error, not a detour
  const size_t lds = ((size_t)kKsWords * K.levels * kKsSamples + 2 * (size_t)kKsKeyRows * kKsCols) * sizeof(u32);
  if (!plan.matrix && lds > 64 * 1024) return hipErrorInvalidValue;
  if (plan.splits > 1) {
    e = hipMemsetAsync(lwe_out, 0, batch * ((size_t)n + 1) * sizeof(u32), s);
    if (e != hipSuccess) return e;
  }
  const dim3 grid(plan.grid_x, plan.grid_y, plan.splits);
  if (plan.matrix)
    hipLaunchKernelGGL(key_switch_matrix_kernel, grid, dim3(256), 0, s, K, ksm_layout(big_n, K.levels, n), lwe_in, batch,
                       static_cast<const uint4*>(ksk_matrix), lwe_out, plan.per_split);
  else
    hipLaunchKernelGGL(key_switch_kernel, grid, dim3(256), lds, s, K, big_n, n, lwe_in, batch, ksk, lwe_out,
                       plan.per_split);
  return hipGetLastError();
}

hipError_t decompose_words(hipStream_t s, u32 log_base, u32 levels, u32 fs, const u32* values,
                           size_t count, u32* digits) {
  const u32 ig = 32 - log_base * levels;
  hipLaunchKernelGGL(decompose_words_kernel, dim3(grid_for(count, 256)), dim3(256), 0, s, log_base,
                     levels, ig, fs, values, count, digits);
  return hipGetLastError();
}

hipError_t decompose_glwe(hipStream_t s, u32 log_base, u32 levels, u32 fs, u32 polys_per_ct,
                          u32 n_coeff, const u32* glwe, size_t batch, u32* digits) {
  const u32 ig = 32 - log_base * levels;
  const size_t total = batch * polys_per_ct * n_coeff;
  hipLaunchKernelGGL(decompose_glwe_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, log_base,
                     levels, ig, fs, polys_per_ct, n_coeff, glwe, total, digits);
  return hipGetLastError();
}

hipError_t switch_modulus(hipStream_t s, const u32* values, size_t count, u32 log_from, u32 log_to,
                          u32* out) {
  hipLaunchKernelGGL(switch_modulus_kernel, dim3(grid_for(count, 256)), dim3(256), 0, s, values,
                     count, log_from, log_to, out);
  return hipGetLastError();
}

hipError_t glwe_mul_monomial(hipStream_t s, u32 log_n, u32 polys_per_ct, const u32* glwe,
                             size_t batch, const i64* monomial_index, u32* out) {
  const size_t total = (batch * polys_per_ct) << log_n;
  hipLaunchKernelGGL(glwe_mul_monomial_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, log_n,
                     polys_per_ct, glwe, total, monomial_index, out);
  return hipGetLastError();
}

hipError_t sample_extract(hipStream_t s, u32 log_n, u32 k, const u32* glwe, size_t batch,
                          u32 sample_index, u32* lwe_out) {
  const size_t total = batch * (((size_t)k << log_n) + 1);
  hipLaunchKernelGGL(sample_extract_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, log_n, k,
                     glwe, batch, sample_index, lwe_out);
  return hipGetLastError();
}

hipError_t stream_copy(hipStream_t s, const void* src, void* dst, size_t bytes) {
  const size_t count = bytes / sizeof(copy_vec4);
  const size_t per_block = 256 * kCopyUnroll;
  hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned)((count + per_block - 1) / per_block)), dim3(256), 0, s,
                     static_cast<const copy_vec4*>(src), static_cast<copy_vec4*>(dst), count);
  return hipGetLastError();
}

hipError_t fft_margin(double* worst, bool reset) {
#if defined(TFHE_FFT_TRACK_ERROR)
  unsigned long long bits = 0;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpyFromSymbol(&bits, HIP_SYMBOL(g_fft_margin_bits), sizeof(bits));
  if (e != hipSuccess) return e;
  if (worst) __builtin_memcpy(worst, &bits, sizeof(bits));
  if (reset) {
    const unsigned long long zero = 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_fft_margin_bits), &zero, sizeof(zero));
  }
  return e;
#else
  (void)worst;
  (void)reset;
  return hipErrorNotSupported;
#endif
}

hipError_t lwe_linear(hipStream_t s, u32 c0, const u32* ct0, u32 c1, const u32* ct1, size_t words,
                      u32* out, size_t words_per_ct, u32 b_add) {
  hipLaunchKernelGGL(lwe_linear_kernel, dim3(grid_for(words, 256)), dim3(256), 0, s, c0, ct0, c1, ct1,
                     words, words_per_ct, b_add, out);
  return hipGetLastError();
}

// How a dense call goes out.  A workgroup owns (query, kDenseOuts outputs, kDenseCols columns): `tiles` of them.  A call
// with few tiles does not fill the chip, so the inputs are split over gridDim.z until the launch reaches
// kDenseTargetWgs workgroups -- one resident round: 20 KiB of LDS per workgroup puts 8 on each of the 256 CUs -- with
// a split of at least 64 inputs and at most 32 splits (the key switch's limits).  A forced split is only held to at
// least one staged step (kDenseRows inputs) per split.  Shares are a multiple of kDenseRows, so the count is recomputed
// from the share: no split is empty.  The rule looks at the shape of the call only; the bits do not depend on it.
constexpr size_t kDenseTargetWgs = 2048;
constexpr u32 kMaxGridYZ = 65535u;
inline bool dense_plan_for(size_t queries, u32 inputs, u32 outputs, u32 words, u32 forced_splits, launch::DensePlanInfo* info) {
  if (queries == 0 || inputs == 0 || outputs == 0 || words == 0) return false;
  const size_t col_tiles = ((size_t)words + kDenseCols - 1) / kDenseCols, out_tiles = ((size_t)outputs + kDenseOuts - 1) / kDenseOuts;
  if ((double)queries * (double)col_tiles > (double)kMaxGrid || out_tiles > kMaxGridYZ) return false;
  const size_t tiles = queries * col_tiles * out_tiles;
  size_t splits = forced_splits;
  if (splits == 0) {
    splits = kDenseTargetWgs / tiles;
    const size_t max_splits = ((size_t)inputs + 63) / 64;
    if (splits > max_splits) splits = max_splits;
    if (splits > 32) splits = 32;
  } else {
    const size_t max_splits = ((size_t)inputs + kDenseRows - 1) / kDenseRows;
    if (splits > max_splits) splits = max_splits;
    if (splits > kMaxGridYZ) splits = kMaxGridYZ;
  }
  if (splits < 1) splits = 1;
  const size_t share = (((size_t)inputs + splits - 1) / splits + kDenseRows - 1) / kDenseRows * kDenseRows;
  splits = ((size_t)inputs + share - 1) / share;
  info->splits = (u32)splits;
  info->rows_per_split = (u32)share;
  info->col_tiles = (u32)col_tiles;
  info->out_tiles = (u32)out_tiles;
  info->workgroups = tiles * splits;
  return true;
}

bool dense_plan(size_t queries, u32 inputs, u32 outputs, u32 words, u32 forced_splits, DensePlanInfo* info) {
  return dense_plan_for(queries, inputs, outputs, words, forced_splits, info);
}

hipError_t lwe_dense(hipStream_t s, const u32* x, size_t queries, u32 inputs, const i32* w, const u32* bias, u32 outputs,
                     u32 words, u32 forced_splits, u32* out) {
  DensePlanInfo plan;
  if (!dense_plan_for(queries, inputs, outputs, words, forced_splits, &plan)) return hipErrorInvalidValue;
  if (plan.splits > 1) {
    hipError_t e = hipMemsetAsync(out, 0, queries * outputs * (size_t)words * sizeof(u32), s);
    if (e != hipSuccess) return e;
  }
  const DenseArgs a{x, w, bias, out, inputs, outputs, words, plan.col_tiles, plan.rows_per_split, plan.splits, 0u};
  const dim3 grid((unsigned)(queries * plan.col_tiles), plan.out_tiles, plan.splits);
  hipLaunchKernelGGL(lwe_dense_kernel, grid, dim3(kDenseThreads), kDenseLdsWords * sizeof(u32), s, a);
  return hipGetLastError();
}

hipError_t dense_tile_rows(hipStream_t s, const u32* in, size_t period, size_t count, u32 words, u32* out) {
  const unsigned grid = (unsigned)(count < ((size_t)1 << 20) ? count : (size_t)1 << 20);
  hipLaunchKernelGGL(dense_tile_rows_kernel, dim3(grid), dim3(256), 0, s, in, period, count, words, out);
  return hipGetLastError();
}

hipError_t extract_step(hipStream_t s, const ExtractStepArgs& a) {
  if (a.total == 0 || a.words == 0 || (a.r_shift | a.d_shift | a.s_shift) > 31u) return hipErrorInvalidValue;
  // a thread owns four words at a time
  hipLaunchKernelGGL(extract_step_kernel, dim3(grid_for((a.total + 3) / 4, kExtractThreads)), dim3(kExtractThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t radix_glue(hipStream_t s, const RadixGlueArgs& a) {
  const size_t rotations = (size_t)a.nt * a.nj * a.rows;
  if (rotations == 0 || a.words == 0 || !a.out || a.nj > kRadixMaxBlocks || (a.acc && (!a.tables || a.acc_words % 4 != 0 || a.log_delta > 31u)))
    return hipErrorInvalidValue;
  // a thread owns one word of a ciphertext, then four of an accumulator
  const size_t work = std::max(rotations * a.words, a.acc ? rotations * (a.acc_words / 4) : (size_t)0);
  hipLaunchKernelGGL(radix_glue_kernel, dim3(grid_for(work, kRadixThreads)), dim3(kRadixThreads), 0, s, a);
  return hipGetLastError();
}

// 16-byte stores where every row, mask run and pointer admits them
static bool seeded_quads(const SeededRowsArgs& a) {
  return a.body_shift >= 2 && a.mask_words % 4 == 0 && a.first_word % kSeededBlockWords == 0 &&
         ((uintptr_t)a.out | (uintptr_t)a.in) % 16 == 0;
}
static bool seeded_rows_ok(const SeededRowsArgs& a) {
  return a.out && a.rows != 0 && a.mask_words != 0 && a.mask_words < (1u << 31) && a.body_shift < 31 &&
         a.rows <= kSeededMaxWords / a.mask_words && a.first_word <= kSeededMaxWords - a.rows * a.mask_words;
}

hipError_t seeded_expand(hipStream_t s, const SeededRowsArgs& a) {
  if (!seeded_rows_ok(a)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)seeded_workgroups(a.first_word, a.rows * a.mask_words));  // at most 2^36 / 4,096
  if (seeded_quads(a))
    hipLaunchKernelGGL(seeded_expand_kernel<4>, grid, dim3(kSeededThreads), 0, s, a);
  else
    hipLaunchKernelGGL(seeded_expand_kernel<1>, grid, dim3(kSeededThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t seeded_compress(hipStream_t s, const SeededRowsArgs& a) {
  if (!seeded_rows_ok(a) || !a.in) return hipErrorInvalidValue;
  const bool quads = seeded_quads(a);
  const dim3 grid(grid_for((size_t)(a.rows << a.body_shift) / (quads ? 4 : 1), kSeededThreads));
  if (quads)
    hipLaunchKernelGGL(seeded_compress_kernel<4>, grid, dim3(kSeededThreads), 0, s, a);
  else
    hipLaunchKernelGGL(seeded_compress_kernel<1>, grid, dim3(kSeededThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t glwe_sparse_extract(hipStream_t s, const u32* glwe, size_t batch, const u32* positions, u32 terms, const i32* coeffs,
                               bool per_sample_sets, u32 tables, u32 log_n, u32 k, u32* out) {
  if (batch == 0 || batch > 0x7FFFFFFFull || tables == 0 || terms == 0 || terms > kSparseMaxTerms || terms > (1u << log_n))
    return hipErrorInvalidValue;
  const size_t lds = ((size_t)(k + 1) << log_n) * sizeof(u32);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  const u32 run = sparse_tables_per_run(batch, tables);
  const dim3 grid((unsigned)batch, (tables + run - 1) / run);
  hipLaunchKernelGGL(glwe_sparse_extract_kernel, grid, dim3(kSparseThreads), lds, s, glwe, positions, coeffs, out,
                     per_sample_sets ? (size_t)tables * terms : (size_t)0, log_n, k, terms, tables, run);
  return hipGetLastError();
}

hipError_t multi_value_coefficients(hipStream_t s, const u32* luts, size_t rows, u32 log_p, i32* coeffs) {
  if (rows == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multi_value_coefficients_kernel, dim3(grid_for(rows * ((1u << log_p) + 1u), 256)), dim3(256), 0, s, luts, rows,
                     log_p, coeffs);
  return hipGetLastError();
}

hipError_t multi_value_constants(hipStream_t s, u32 log_p, u32 log_n, u32 k, u32 kappa, u32* acc, u32* positions) {
  if (log_p >= log_n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multi_value_constants_kernel, dim3(grid_for((size_t)(k + 1) << log_n, 256)), dim3(256), 0, s, log_p, log_n, k,
                     kappa, acc, positions);
  return hipGetLastError();
}

hipError_t sparse_positions(hipStream_t s, const u32* host_positions, u32 terms, u32* dst) {
  if (terms == 0 || terms > kSparseMaxTerms) return hipErrorInvalidValue;
  for (u32 at = 0; at < terms; at += kSparsePositionsPerLaunch) {
    SparsePositions p{};
    const u32 count = terms - at < kSparsePositionsPerLaunch ? terms - at : kSparsePositionsPerLaunch;
    for (u32 i = 0; i < count; ++i) p.v[i] = host_positions[at + i];
    hipLaunchKernelGGL(sparse_positions_kernel, dim3(1), dim3(64), 0, s, p, count, dst + at);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// How a convolution goes out: one team per (query, output); the channels in passes of rows_per_pass, the admitted
// maximum (or the forced count) held to the channels there are.  The words do not depend on it.
bool glwe_conv_plan(size_t queries, u32 channels, u32 outputs, u32 admitted_rows, u32 forced_rows, GlweConvPlanInfo* info) {
  if (queries == 0 || channels == 0 || outputs == 0 || admitted_rows == 0 || forced_rows > admitted_rows) return false;
  if ((double)queries * (double)outputs > (double)kMaxGrid) return false;
  u32 rows = forced_rows ? forced_rows : admitted_rows;
  if (rows > channels) rows = channels;
  info->rows_per_pass = rows;
  info->passes = (channels + rows - 1) / rows;
  info->teams = queries * outputs;
  return true;
}

hipError_t conv_weights(hipStream_t s, int field, u32 log_n, const void* tw, const i32* polys, size_t poly_count, void* spectra) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN(log_n, (launch_conv_weights<FF, LL>(s, tw, polys, poly_count, spectra))));
}

hipError_t glwe_conv(hipStream_t s, int field, u32 log_n, u32 k, const void* tw, const GlweConvArgs& args, size_t queries) {
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN_K(log_n, k, (launch_glwe_conv<FF, LL, KK>(s, tw, args, queries))));
}

hipError_t sample_extract_indices(hipStream_t s, u32 log_n, u32 k, const u32* glwe, size_t batch, const u32* indices,
                                  size_t count, u32* lwe_out) {
  const size_t total = batch * count * ((size_t)k * ((size_t)1 << log_n) + 1);
  hipLaunchKernelGGL(sample_extract_indices_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, log_n, k, glwe, batch, indices,
                     count, lwe_out);
  return hipGetLastError();
}

hipError_t glwe_body(hipStream_t s, int field, u32 log_n, const void* tw, u32 k, const u32* rows,
                     size_t row_count, const u32* sk, u32* dst, size_t dst_stride, bool negate) {
  if (row_count == 0) return hipSuccess;
  TFHE_DISPATCH_FIELD(field, TFHE_DISPATCH_LOGN(log_n, (launch_glwe_body<FF, LL>(s, tw, k, rows, row_count, sk, dst, dst_stride, negate ? 1u : 0u))));
}

hipError_t lwe_body(hipStream_t s, const u32* rows, size_t row_count, u32 n, const u32* sk,
                    const u32* plaintext, u32* dst, size_t dst_stride, bool negate) {
  if (row_count == 0) return hipSuccess;
  const unsigned grid = (unsigned)((row_count + 3) / 4);
  hipLaunchKernelGGL(lwe_body_kernel, dim3(grid), dim3(256), 0, s, rows, row_count, n, sk, plaintext,
                     dst, dst_stride, negate ? 1u : 0u);
  return hipGetLastError();
}

hipError_t ggsw_add_gadget(hipStream_t s, u32* ggsw, size_t ggsw_count, u32 k, u32 log_n, u32 levels,
                           u32 log_base, u32 gadget_top, const u32* messages) {
  const size_t total = ggsw_count * (size_t)(k + 1) * levels;
  hipLaunchKernelGGL(ggsw_add_gadget_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, ggsw,
                     ggsw_count, k, log_n, levels, log_base, gadget_top, messages);
  return hipGetLastError();
}

}  // namespace launch
}  // namespace tfhe
