// launch.h -- host-callable launchers of the gfx950 kernels (implemented in kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "block_rotate.h"
#include "glwe_conv.h"
#include "glwe_switch.h"
#include "ks_matrix.h"
#include "lwe_extract.h"
#include "multi_value.h"
#include "multibit.h"
#include "pbs_wave.h"
#include "radix.h"
#include "seeded.h"

namespace tfhe {
namespace launch {

// NTT backends (field policies): values of the `field` argument below
constexpr int kFieldGoldilocks = GlField::kId;  // 1
constexpr int kFieldFp64 = FpField::kId;        // 2
constexpr int kFieldGoldilocksSplit = GlSplitField::kId;  // 3
constexpr int kFieldFp49 = Fp49Field::kId;                // 4
constexpr int kFieldFft = FftField::kId;                  // 5: complex FFT in fp64, exact by a rounding bound

// true if a kernel set is instantiated for (log_n, k)
bool shape_supported(u32 log_n, u32 k);
// spectra per key polynomial for a field (1 or 2)
int field_parts(int field);
// true if the field's kernels exist at this ring degree
bool field_shape_supported(int field, u32 log_n);
// samples a team of the blind-rotation kernel rotates at once for (field, log_n, k): 1 or 2
int samples_per_team(int field, u32 log_n, u32 k);

// twiddle table psi_rev[N] (8-byte field elements) must already be on the device;
// spectra: poly_count x field_parts x N elements; k (the GLWE dimension) selects the key's layout with log_n and the
// field (pbs_wave.h::key_layout_e: the pair kernel's at N = 512, k = 1 in the complex transform)
hipError_t bsk_prepare(hipStream_t s, int field, u32 log_n, u32 k, const void* tw, const u32* polys,
                       size_t poly_count, void* spectra);

// A second stream of the caller's, with the two events that fork it from and join it to the main one: batches larger than
// what the chip holds at once go out as two halves whose segment launches alternate (kernels.hip::blind_rotate_plan).
struct SideStream {
  hipStream_t stream;
  hipEvent_t fork, join;
};

// Kernel shape of a blind rotation (tfhe_context_set_kernel_shape): the launcher's own choice by batch size, the wide
// team (2 (k+1) waves per sample: the latency shape, complex transform up to N = 1024) wherever it is offered, or
// always the throughput team
constexpr int kShapeAuto = 0, kShapeWide = 1, kShapeTeam = 2;

// Blind rotation of `batch` samples.  Optional outputs: glwe_out [batch][k+1][N] and/or
// lwe_extracted [batch][k*N+1] (sample extract at index 0 fused in).
// `state`: [batch][k+1][N] words of scratch that hold the accumulators between the launches of a segmented rotation
// (may be glwe_out itself; null: one launch per rotation).  `side`: null = everything on s.  On return all work is
// ordered on s (the side stream has been joined).
hipError_t blind_rotate(hipStream_t s, int field, const PbsParams& P, const void* tw,
                        const u32* lwe_in, size_t batch, const u32* tv, size_t tv_stride,
                        const void* bsk, u32* glwe_out, u32* lwe_extracted, u32* state = nullptr,
                        const SideStream* side = nullptr, int shape = kShapeAuto);

// How blind_rotate would send out a batch (kernels.hip::blind_rotate_plan), for bench lines and tests
struct BlindRotatePlanInfo {
  size_t chunk;             // samples per group of launches
  u32 segments;             // launches per rotation (key slices)
  int streams;              // 1 or 2
  size_t resident_samples;  // samples the chip rotates at once (teams it holds x samples per team)
  int samples_per_team;
  int waves_per_sample;     // K+1 groups of G waves (shared by samples_per_team samples), or 2 (K+1) for the wide team
};
hipError_t blind_rotate_plan(int field, const PbsParams& P, size_t batch, bool can_park, bool have_side,
                             BlindRotatePlanInfo* out, int shape = kShapeAuto);

// The unrolled blind rotation of notes/BMMP Bootstrapping.md (two key bits per step): bsk holds
// n/2 * 3 prepared GGSWs (pbs_wave.h::blind_rotate_bmmp_team); n even, shape_supported_bmmp only.
bool shape_supported_bmmp(u32 log_n, u32 k);
bool field_supported_bmmp(int field);  // Goldilocks and fp64-p49: the fields whose BMMP kernel does not lose to the loop
hipError_t blind_rotate_bmmp(hipStream_t s, int field, const PbsParams& P, const void* tw,
                             const u32* lwe_in, size_t batch, const u32* tv, size_t tv_stride,
                             const void* bsk, u32* glwe_out, u32* lwe_extracted);

// ---- multi-bit blind rotation (multibit.h): g key bits per external product, offered where the wide team is.
// *why = 0 where (field, P) is offered, else which of its conditions fails
constexpr int kMultibitNoBackend = 1, kMultibitNoRing = 2, kMultibitNoLds = 3;  // not the complex transform / N > 1024 / the row buffers
hipError_t multibit_refusal(int field, const PbsParams& P, int* why);
// bundles [batch][ceil(n / g)] prepared GGSWs (the layout of a bootstrapping key for P.k) from the raw key
// [ceil(n / g)][2^g - 1][(k+1) l][k+1][N] and lwe_in [batch][n+1]: one launch of (polynomials, batch) workgroups.
// hipErrorInvalidValue: g outside {2, 3, 4}, an empty batch, one beyond 65535, a shape that is not offered
hipError_t multibit_bundle(hipStream_t s, int field, const PbsParams& P, const void* tw, const u32* key, u32 g, const u32* lwe_in,
                           size_t batch, void* bundles);
// the rotation over `groups` bundles per sample, one wide team per sample; tv, tv_stride, P.acc_glwe / P.acc_offset and
// the optional outputs as for blind_rotate
hipError_t multibit_rotate(hipStream_t s, int field, const PbsParams& P, const void* tw, const u32* lwe_in, size_t batch, const u32* tv,
                           size_t tv_stride, const void* bundles, u32 groups, u32* glwe_out, u32* lwe_extracted);

// ---- block-binary blind rotation (block_rotate.h): `block` key bits per decomposition on the loaded, ordinary key.
// Offered for the complex transform at N = 512 and 1024 (one wave per polynomial).  One team of k+1 waves per sample at
// EVERY batch: the batches blind_rotate gives to the wide team or the pair kernel run on this team kernel too.
bool block_rotate_supported(int field, u32 log_n, u32 k);
// `roots`: block_root_words(log_n) elements of fill_block_roots on the device.  Chunks, segments and streams as
// blind_rotate sends them out (the same plan), segment lengths rounded up to a multiple of `block`; `state` and `side` as there.
hipError_t block_rotate(hipStream_t s, int field, const PbsParams& P, const void* tw, const void* roots, const u32* lwe_in, size_t batch,
                        const u32* tv, size_t tv_stride, const void* bsk, u32 block, u32* glwe_out, u32* lwe_extracted,
                        u32* state = nullptr, const SideStream* side = nullptr);

// out = external_product(ggsw[g], glwe[b]) (+ ct0 for the CMUX form).
//   cmux_ct0 == nullptr : src = glwe_in
//   cmux_ct0 != nullptr : src = ct1 - ct0 where ct1 = glwe_inout_ct1 (overwritten with the
//                         difference, ggsw.rs:171), out = product + ct0
hipError_t external_product(hipStream_t s, int field, const PbsParams& P, const void* tw,
                            const void* ggsw, size_t ggsw_stride_words, const u32* glwe_in,
                            u32* ct1_inout, const u32* cmux_ct0, size_t batch, u32* glwe_out,
                            unsigned long long* queue /* one device word of scratch: ticket counter of long batches */);

// Path of a key switch (tfhe_context_set_key_switch_path): the launcher's own choice, always the u32 multiply-add
// kernel, or always the int8 matrix-core kernel over the prepared key (ks_matrix.h; only where ksm_admitted)
constexpr int kKsPathAuto = 0, kKsPathScalar = 1, kKsPathMatrix = 2;
// How key_switch would send out a batch.  hipErrorInvalidValue: kKsPathMatrix on a decomposer that is not admitted.
struct KeySwitchPlanInfo {
  bool matrix;
  unsigned grid_x, grid_y;  // column tiles and sample tiles of workgroups
  unsigned splits;          // gridDim.z; more than one: the output is zeroed first, partial sums are added
  u32 per_split;            // mask words (scalar) or 32-word super-blocks (matrix) per split
};
hipError_t key_switch_plan(const KsParams& K, u32 big_n, u32 n, size_t batch, int path, KeySwitchPlanInfo* out);
// the prepared key of the matrix path: bytes, and ksk [big_n*levels][n+1] -> prepared
size_t ksk_matrix_bytes(const KsParams& K, u32 big_n, u32 n);
hipError_t ksk_prepare_matrix(hipStream_t s, const KsParams& K, u32 big_n, u32 n, const u32* ksk, void* prepared);
// key_switch_lwe over a batch: lwe_in [batch][big_n+1], ksk [big_n*levels][n+1], out [batch][n+1]; ksk_matrix: the
// same key prepared by ksk_prepare_matrix (may be null with kKsPathScalar)
hipError_t key_switch(hipStream_t s, const KsParams& K, u32 big_n, u32 n, const u32* lwe_in,
                      size_t batch, const u32* ksk, u32* lwe_out, const void* ksk_matrix, int path);

// ---- packing key switch (pbs_wave.h::pack_lwe_team): `groups` outputs of up to N LWE ciphertexts of dimension d each
// cols [groups][d+1][N] = the transposed ciphertexts of lwe_in [groups][per_group][d+1], zero above per_group
// log_rep > 0: the replicated layout of the tree LUT -- lwe_in [groups][per_group][d+1] with per_group = N >> log_rep,
// cols[g][i][j] = lwe_in[g][j >> log_rep][i] (the same bits as the plain transpose of the materialised N-fold list)
hipError_t pack_transpose(hipStream_t s, const u32* lwe_in, size_t groups, u32 per_group, u32 d, u32 log_n, u32* cols,
                          u32 log_rep = 0);
// glwe_out [groups][k+1][N] (ZEROED by the caller, on s) += the packed ciphertexts.  P: log_n, k and the KS decomposer
// in log_base / levels / ignored_bits / first_shift; key: the packing key prepared by bsk_prepare(.., k, ..) as
// ceil(d / (k+1)) GGSW-shaped slices of (k+1) l_ks rows (rows past d l_ks zero-filled)
hipError_t pack_lwe(hipStream_t s, int field, const PbsParams& P, const void* tw, const void* key, const u32* cols, u32 d,
                    size_t groups, u32* glwe_out);
// pksk [rows][k+1][N]: body coefficient 0 of row r += factor[r]
hipError_t packing_add_gadget(hipStream_t s, u32* pksk, size_t rows, u32 k, u32 log_n, const u32* factor);

// ---- GLWE key switch / automorphism (glwe_switch.h::glwe_switch_team): glwe_out [batch][k+1][N] = Auto_t(glwe_in[b]; key)
// (+ glwe_in[b] with add_input), one launch of `batch` teams; t_inv = t^-1 mod 2N.  P as for pack_lwe; key: the switch
// key [k l_ks][k+1][N] prepared by bsk_prepare(.., k, ..) followed by l_ks (k+1) zero spectra (one packing slice of
// dimension k).  glwe_out may be glwe_in.  hipErrorInvalidValue: an empty batch, one of 2^31 or more, an even t_inv
hipError_t glwe_switch(hipStream_t s, int field, const PbsParams& P, const void* tw, const void* key, const u32* glwe_in,
                       size_t batch, u32 t_inv, bool add_input, u32* glwe_out);
// the bare permutation of `polys` polynomials [N] (glwe_switch.h::automorphism_poly); glwe_out may be glwe_in
hipError_t glwe_automorphism(hipStream_t s, const u32* glwe_in, size_t polys, u32 log_n, u32 t_inv, u32* glwe_out);
// key [k levels][k+1][N]: the body of row i levels + l += from_polys[i] (device, [k][N], entries in {-1, 0, 1}) times
// 2^(top - log_base (l + 1))
hipError_t glwe_switch_add_gadget(hipStream_t s, u32* key, u32 k, u32 log_n, u32 levels, u32 log_base, u32 top,
                                  const i32* from_polys);

// ---- tree LUT (capi.cpp::tfhe_tree_lut_batch_device): the per-rotation inputs of a level, in the reserved workspace
// out [count][words], out[r] = in[r / per_row]: rotation r's copy of its row's digit
hipError_t tree_lut_expand(hipStream_t s, const u32* in, size_t count, size_t per_row, u32 words, u32* out);
// tv [count][N], tv[r] = construct_test_from_lut of the 2^log_p table entries at table + (r / per_row) * set_stride +
// (r % per_row) * 2^log_p (set_stride 0: every row reads the one shared set); un-encoded
hipError_t tree_lut_test_vectors(hipStream_t s, const u32* table, size_t set_stride, size_t count, size_t per_row, u32 log_p,
                                 u32 log_n, u32* tv);

// ---- CMUX tree / encrypted table lookup (pbs_wave.h::cmux_tree_team), DEMUX tree / encrypted table update
// (demux_tree_team) and encrypted branching program (cmux_program_team).  Which passes go out is host arithmetic
// (passes.h); here is what needs the device: the teams of a feature's kernel the current device holds at once (the
// automatic rules' `resident`), and the launch of one pass.  pass.query_stride in 8-byte words here.
hipError_t tree_resident_teams(int field, const PbsParams& P, unsigned* out);
// `teams` = trees << pass.log_subtrees workgroups
hipError_t cmux_tree_pass(hipStream_t s, int field, const PbsParams& P, const void* tw, const CmuxTreePass& pass, size_t teams);
hipError_t demux_resident_teams(int field, const PbsParams& P, unsigned* out);
// `teams` = trees << pass.log_subtrees workgroups
hipError_t demux_tree_pass(hipStream_t s, int field, const PbsParams& P, const void* tw, const DemuxTreePass& pass, size_t teams);
hipError_t program_resident_teams(int field, const PbsParams& P, unsigned* out);
// queries * pass.parts workgroups
hipError_t cmux_program_pass(hipStream_t s, int field, const PbsParams& P, const void* tw, const CmuxProgramPass& pass, size_t queries);

// ---- dense layer (lwe_dense.h::dense_tile; the plan: kernels.hip::dense_plan_for)
struct DensePlanInfo {
  u32 splits;          // shares of the inputs (gridDim.z); more than one: the output is zeroed first, partial sums are added
  u32 rows_per_split;  // inputs per share, a multiple of the staged rows
  u32 col_tiles, out_tiles;
  size_t workgroups;   // queries * col_tiles * out_tiles * splits
};
// forced_splits 0: automatic.  false: a size is 0 or the tiles exceed the grid (queries * col_tiles < 2^31, out_tiles < 2^16)
bool dense_plan(size_t queries, u32 inputs, u32 outputs, u32 words, u32 forced_splits, DensePlanInfo* info);
// out[q][o][c] = sum_i (u32)w[o][i] x[q][i][c] mod 2^32, bias[o] (may be null) added to word `words - 1` (a memset node
// and one launch, or one launch).  hipErrorInvalidValue: see dense_plan
hipError_t lwe_dense(hipStream_t s, const u32* x, size_t queries, u32 inputs, const i32* w, const u32* bias, u32 outputs,
                     u32 words, u32 forced_splits, u32* out);
// out [count][words], out[r] = in[r % period]: the per-neuron test vectors of a fused layer, one per bootstrap
hipError_t dense_tile_rows(hipStream_t s, const u32* in, size_t period, size_t count, u32 words, u32* out);

// ---- digit extraction (lwe_extract.h::extract_step): the one elementwise launch between two sign bootstraps.
// hipErrorInvalidValue: an empty call or a shift above 31
hipError_t extract_step(hipStream_t s, const ExtractStepArgs& a);

// ---- radix integers (radix.h::radix_glue): the one elementwise launch in front of a bootstrap level.
// hipErrorInvalidValue: no rotation, more than kRadixMaxBlocks blocks, accumulators without tables
hipError_t radix_glue(hipStream_t s, const RadixGlueArgs& a);

// ---- seeded ciphertexts (seeded.h): rows of mask_words mask words and 2^body_shift body words.  seeded_expand writes
// the masks from the stream (and the bodies from a.in, unless null); seeded_compress gathers the bodies of a.in into a.out.
// hipErrorInvalidValue: no row, no mask word, a null pointer, a word range past 2^36
hipError_t seeded_expand(hipStream_t s, const SeededRowsArgs& a);
hipError_t seeded_compress(hipStream_t s, const SeededRowsArgs& a);

// ---- multi-value bootstrap (multi_value.h::sparse_extract_tile): out [batch][tables][k N + 1], the signed gather of
// `terms` sample extractions of glwe [batch][k+1][N] at positions [terms] (device) times coeffs [1 or batch][tables][terms].
// One workgroup per (sample, run of tables): multi_value.h::sparse_tables_per_run.
// hipErrorInvalidValue: an empty call, more than kSparseMaxTerms or N terms, a ring whose GLWE exceeds 64 KiB of LDS
hipError_t glwe_sparse_extract(hipStream_t s, const u32* glwe, size_t batch, const u32* positions, u32 terms, const i32* coeffs,
                               bool per_sample_sets, u32 tables, u32 log_n, u32 k, u32* out);
// coeffs [rows][B + 1] = multi_value_coefficient(luts [rows][B])
hipError_t multi_value_coefficients(hipStream_t s, const u32* luts, size_t rows, u32 log_p, i32* coeffs);
// acc [k+1][N] = (0, .., 0, kappa (1 + X + .. + X^(N-1))), positions [B + 1] = multi_value_position
hipError_t multi_value_constants(hipStream_t s, u32 log_p, u32 log_n, u32 k, u32 kappa, u32* acc, u32* positions);
// dst [terms] (device) = host_positions, as kernel arguments: no copy node, capturable
hipError_t sparse_positions(hipStream_t s, const u32* host_positions, u32 terms, u32* dst);

// ---- encrypted convolution (glwe_conv.h::glwe_conv_team; the plan: kernels.hip::glwe_conv_plan)
struct GlweConvPlanInfo {
  u32 rows_per_pass;  // channels summed in the transform domain before a lift
  u32 passes;         // ceil(channels / rows_per_pass)
  size_t teams;       // queries * outputs workgroups
};
// admitted_rows: what the backend's exactness rule admits at the weights' magnitude (capi.cpp::conv_rows_admitted);
// forced_rows 0: automatic.  false: a size is 0, forced_rows exceeds admitted_rows, or queries * outputs >= 2^31
bool glwe_conv_plan(size_t queries, u32 channels, u32 outputs, u32 admitted_rows, u32 forced_rows, GlweConvPlanInfo* info);
// spectra [poly_count][N >> kLogShrink] field elements (8 N bytes each at most) = the transformed weight polynomials [poly_count][N]
hipError_t conv_weights(hipStream_t s, int field, u32 log_n, const void* tw, const i32* polys, size_t poly_count, void* spectra);
// args.x_spec: the call's ciphertext polynomials prepared by bsk_prepare(.., k, ..); one launch of queries * outputs teams
hipError_t glwe_conv(hipStream_t s, int field, u32 log_n, u32 k, const void* tw, const GlweConvArgs& args, size_t queries);
// lwe_out [batch][count][k N + 1] = sample_extract(glwe[b], indices[i]); indices [count] on the device, each below N
hipError_t sample_extract_indices(hipStream_t s, u32 log_n, u32 k, const u32* glwe, size_t batch, const u32* indices,
                                  size_t count, u32* lwe_out);

// elementwise helpers.  first_shift = bit of the lowest kept limb (PbsParams::first_shift)
hipError_t decompose_words(hipStream_t s, u32 log_base, u32 levels, u32 first_shift, const u32* values,
                           size_t count, u32* digits /* [count][levels] */);
hipError_t decompose_glwe(hipStream_t s, u32 log_base, u32 levels, u32 first_shift, u32 polys_per_ct,
                          u32 n_coeff, const u32* glwe, size_t batch,
                          u32* digits /* [batch][polys*levels][N] */);
hipError_t switch_modulus(hipStream_t s, const u32* values, size_t count, u32 log_from, u32 log_to,
                          u32* out);
hipError_t glwe_mul_monomial(hipStream_t s, u32 log_n, u32 polys_per_ct, const u32* glwe,
                             size_t batch, const i64* monomial_index, u32* out);
hipError_t sample_extract(hipStream_t s, u32 log_n, u32 k, const u32* glwe, size_t batch,
                          u32 sample_index, u32* lwe_out);
// out = c0*ct0 + c1*ct1 (ct1 may be null when c1 == 0); lwe.rs:9-23, boolean.rs:18.  With
// words_per_ct != 0, b_add is added to the b slot (last word) of every ciphertext.
hipError_t lwe_linear(hipStream_t s, u32 c0, const u32* ct0, u32 c1, const u32* ct1, size_t words,
                      u32* out, size_t words_per_ct = 0, u32 b_add = 0);

// ---- encryption side (keygen / encrypt / decrypt with caller-supplied randomness)
// dst[row][j] = body(rows[row])[j] +/- sum_i masks(rows[row])[i] (*) sk[i]; rows [row_count][k+1][N],
// sk [k][N] binary, dst rows of dst_stride words (may alias the bodies)
hipError_t glwe_body(hipStream_t s, int field, u32 log_n, const void* tw, u32 k, const u32* rows,
                     size_t row_count, const u32* sk, u32* dst, size_t dst_stride, bool negate);
// dst[row*dst_stride] = rows[row][n] +/- <rows[row][0..n), sk> (+ plaintext[row] if non-null)
hipError_t lwe_body(hipStream_t s, const u32* rows, size_t row_count, u32 n, const u32* sk,
                    const u32* plaintext, u32* dst, size_t dst_stride, bool negate);
// ggsw.rs:96-103 for ggsw_count matrices [(k+1)*levels][k+1][N]
hipError_t ggsw_add_gadget(hipStream_t s, u32* ggsw, size_t ggsw_count, u32 k, u32 log_n, u32 levels,
                           u32 log_base, u32 gadget_top, const u32* messages);

// Probe builds (-DTFHE_FFT_TRACK_ERROR, libtfhe_hip_probe.so): largest |value - nearest integer| the complex
// transform has lifted on the device since the last reset.  The product build has no probe: hipErrorNotSupported.
hipError_t fft_margin(double* worst, bool reset);

// dst[0..bytes) = src[0..bytes) with 16-byte accesses (bytes a multiple of 16): HBM roofline probe
hipError_t stream_copy(hipStream_t s, const void* src, void* dst, size_t bytes);

}  // namespace launch
}  // namespace tfhe
