//! Rust-side binding a maintainer of Janmajayamall/tfhe-research would add to call the MI355X
//! engine from the crate, keeping the crate-internal signatures of the bootstrapping path.
//! SOURCE ONLY (never compiled here: no Rust toolchain in the image).  The C ABI is
//! `include/tfhe_hip.h`; everything below is plumbing between ndarray buffers and raw pointers.
//!
//! Reference signatures mirrored (file:line under src/):
//!   bootstrap            bootstrapping.rs:58-65
//!   key_switch_lwe       key_switching.rs:63-69
//!   external_product     ggsw.rs:132-136        cmux   ggsw.rs:164-169
//!   and / or             boolean.rs:9-14, 32-37
//!   construct_test_from_lut  test_vector.rs:38
//!   bootstrapping_key_gen    bootstrapping.rs:23-28   encrypt_lwe_plaintext / decrypt_lwe  lwe.rs:138-173
use ndarray::{Array1, Array2, Array3};
use std::os::raw::{c_char, c_int, c_uint, c_void};

#[repr(C)]
#[derive(Clone, Copy)]
pub struct CDecomposerParams { pub log_base: u32, pub levels: u32, pub log_q: u32 }

#[repr(C)]
#[derive(Clone, Copy)]
pub struct CTfheParams {
    pub glwe_dimension: u32, pub glwe_poly_degree: u32, pub lwe_dimension: u32,
    pub padding_bits: u32, pub log_p: u32, pub log_q: u32,
    pub ks_decomposer: CDecomposerParams, pub pbs_decomposer: CDecomposerParams,
}

#[repr(C)] pub struct TfheContext { _private: [u8; 0] }
#[repr(C)] pub struct TfhePolyWeights { _private: [u8; 0] }
#[repr(C)] pub struct TfheGlweSwitchKey { _private: [u8; 0] }
#[repr(C)] pub struct TfheMultibitKey { _private: [u8; 0] }
#[repr(C)] pub struct TfhePool { _private: [u8; 0] }

extern "C" {
    // multi-GPU pool (include/tfhe_hip.h, "multi-GPU pool"): one context per listed HIP device, ONE key prepared
    // once and replicated device to device, batches cut into contiguous slices
    fn tfhe_pool_create(params: *const CTfheParams, devices: *const c_int, n_devices: usize, backend: c_int,
                        out: *mut *mut TfhePool) -> c_int;
    fn tfhe_pool_destroy(pool: *mut TfhePool);
    fn tfhe_pool_member(pool: *mut TfhePool, i: usize) -> *mut TfheContext;
    fn tfhe_pool_last_error(pool: *const TfhePool) -> *const c_char;
    fn tfhe_pool_load_bootstrapping_key(pool: *mut TfhePool, bsk: *const u32, ksk: *const u32) -> c_int;
    fn tfhe_pool_load_bootstrapping_key_bmmp(pool: *mut TfhePool, bsk_bmmp: *const u32, ksk: *const u32) -> c_int;
    fn tfhe_pool_bootstrap_batch(pool: *mut TfhePool, lwe_in: *const u32, batch: usize,
                                 test_vector_poly: *const u32, tv_count: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_pool_gate_batch(pool: *mut TfhePool, truth: *const u32, ct0: *const u32, ct1: *const u32,
                            batch: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_pool_set_kernel_shape(pool: *mut TfhePool, shape: c_int) -> c_int;
    fn tfhe_pool_set_key_switch_path(pool: *mut TfhePool, path: c_int) -> c_int;
    fn tfhe_last_error(ctx: *const TfheContext) -> *const c_char;
    fn tfhe_bootstrap_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize,
                            test_vector_poly: *const u32, tv_count: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_key_switch_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_external_product_batch(ctx: *mut TfheContext, ggsw: *const u32, ggsw_count: usize,
                                   glwe_in: *const u32, batch: usize, glwe_out: *mut u32) -> c_int;
    // packing key switch (include/tfhe_hip.h): many LWE results into one GLWE ciphertext
    fn tfhe_generate_packing_key(ctx: *mut TfheContext, from_sk: *const u32, from_dimension: usize,
                                 glwe_sk: *const u32, pksk: *mut u32) -> c_int;
    fn tfhe_load_packing_key(ctx: *mut TfheContext, pksk: *const u32, from_dimension: usize) -> c_int;
    fn tfhe_packing_key_dimension(ctx: *const TfheContext, from_dimension: *mut usize) -> c_int;
    fn tfhe_pack_lwe_batch(ctx: *mut TfheContext, lwe_in: *const u32, groups: usize, per_group: usize,
                           glwe_out: *mut u32) -> c_int;
    // CMUX tree / encrypted table lookup (include/tfhe_hip.h)
    fn tfhe_cmux_tree(ctx: *mut TfheContext, selectors: *const u32, queries: usize, depth: usize, leaves: *const u32,
                      leaf_sets: usize, tables: usize, glwe_out: *mut u32) -> c_int;
    fn tfhe_table_lookup(ctx: *mut TfheContext, selectors: *const u32, queries: usize, depth: usize, table: *const u32,
                         table_sets: usize, tables: usize, lwe_out: *mut u32) -> c_int;
    // encrypted branching program (include/tfhe_hip.h)
    fn tfhe_cmux_program(ctx: *mut TfheContext, selectors: *const u32, queries: usize, n_inputs: usize, selector_sets: usize,
                         nodes: *const ProgramNode, n_nodes: usize, terminals: *const u32, n_terminals: usize,
                         outputs: *const u32, n_outputs: usize, glwe_out: *mut u32, lwe_out: *mut u32) -> c_int;
    // DEMUX tree / encrypted table update (include/tfhe_hip.h)
    fn tfhe_demux_tree(ctx: *mut TfheContext, selectors: *const u32, queries: usize, depth: usize, glwe_in: *const u32,
                       values: usize, leaves_out: *mut u32, leaf_sets: usize, accumulate: c_int) -> c_int;
    fn tfhe_table_write(ctx: *mut TfheContext, selectors: *const u32, queries: usize, depth: usize, values: *const u32,
                        table_inout: *mut u32, table_sets: usize, tables: usize) -> c_int;
    fn tfhe_table_lookup_glwe(ctx: *mut TfheContext, selectors: *const u32, queries: usize, depth: usize, leaves: *const u32,
                              leaf_sets: usize, tables: usize, lwe_out: *mut u32) -> c_int;
    // rotation from a GLWE accumulator and the tree LUT (include/tfhe_hip.h)
    fn tfhe_blind_rotate_glwe_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize, acc_in: *const u32,
                                    acc_count: usize, rotation_offset: usize, glwe_out: *mut u32) -> c_int;
    fn tfhe_bootstrap_glwe_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize, acc_in: *const u32,
                                 acc_count: usize, rotation_offset: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_tree_lut_batch(ctx: *mut TfheContext, digits: *const *const u32, d: usize, batch: usize, table: *const u32,
                           table_sets: usize, tables: usize, lwe_out: *mut u32) -> c_int;
    // digit extraction and the wide LUT (include/tfhe_hip.h)
    fn tfhe_extract_digits_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize, lsb: c_uint, digit_bits: c_uint,
                                 digits: c_uint, out_lsb: c_uint, digits_out: *const *mut u32, remainder_out: *mut u32) -> c_int;
    fn tfhe_wide_lut_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize, lsb: c_uint, d: usize, table: *const u32,
                           table_sets: usize, tables: usize, lwe_out: *mut u32) -> c_int;
    // radix integers (include/tfhe_hip.h)
    fn tfhe_radix_propagate_batch(ctx: *mut TfheContext, blocks_in: *const u32, batch: usize, blocks: usize, blocks_out: *mut u32) -> c_int;
    fn tfhe_radix_map_batch(ctx: *mut TfheContext, a: *const u32, a_blocks: usize, wa: u32, a_shift: i32, a_fixed: i32, b: *const u32,
                            b_blocks: usize, wb: u32, b_shift: i32, b_fixed: i32, batch: usize, blocks: usize, tables: *const u32,
                            table_count: usize, table_of_block: *const u32, out: *mut u32) -> c_int;
    fn tfhe_radix_compare_batch(ctx: *mut TfheContext, a: *const u32, b: *const u32, batch: usize, blocks: usize, predicate: c_uint,
                                out: *mut u32) -> c_int;
    // seeded ciphertexts and compressed keys (include/tfhe_hip.h)
    fn tfhe_seed_words(seed: *const TfheSeed, domain: u32, first_word: u64, count: usize, out: *mut u32) -> c_int;
    fn tfhe_expand_lwe_rows(ctx: *mut TfheContext, seed: *const TfheSeed, bodies: *const u32, first_row: u64, rows: usize, dimension: usize,
                            lwe_out: *mut u32) -> c_int;
    fn tfhe_expand_glwe_rows(ctx: *mut TfheContext, seed: *const TfheSeed, bodies: *const u32, first_row: u64, rows: usize,
                             glwe_out: *mut u32) -> c_int;
    fn tfhe_compress_lwe_rows(ctx: *mut TfheContext, lwe: *const u32, rows: usize, dimension: usize, bodies_out: *mut u32) -> c_int;
    fn tfhe_compress_glwe_rows(ctx: *mut TfheContext, glwe: *const u32, rows: usize, bodies_out: *mut u32) -> c_int;
    fn tfhe_load_bootstrapping_key_seeded(ctx: *mut TfheContext, bsk_seed: *const TfheSeed, bsk_bodies: *const u32, ksk_seed: *const TfheSeed,
                                          ksk_bodies: *const u32) -> c_int;
    fn tfhe_bootstrap_batch_seeded(ctx: *mut TfheContext, seed: *const TfheSeed, first_row: u64, bodies: *const u32, batch: usize,
                                   test_vector_poly: *const u32, tv_count: usize, lwe_out: *mut u32) -> c_int;
    // multi-value bootstrapping (include/tfhe_hip.h)
    fn tfhe_multi_value_bootstrap_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize, luts: *const u32, lut_sets: usize,
                                        tables: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_glwe_sparse_extract_batch(ctx: *mut TfheContext, glwe: *const u32, batch: usize, positions: *const u32, terms: usize,
                                      coeffs: *const i32, sets: usize, tables: usize, lwe_out: *mut u32) -> c_int;
    // encrypted dense layers (include/tfhe_hip.h)
    fn tfhe_lwe_dense_batch(ctx: *mut TfheContext, x: *const u32, queries: usize, inputs: usize, weights: *const i32,
                            bias: *const u32, outputs: usize, words_per_ct: usize, out: *mut u32) -> c_int;
    fn tfhe_dense_bootstrap_batch(ctx: *mut TfheContext, x: *const u32, queries: usize, inputs: usize, weights: *const i32,
                                  bias: *const u32, outputs: usize, test_vector_poly: *const u32, tv_count: usize,
                                  lwe_out: *mut u32) -> c_int;
    // encrypted convolutions (include/tfhe_hip.h)
    fn tfhe_prepare_poly_weights(ctx: *mut TfheContext, weights: *const i32, outputs: usize, channels: usize,
                                 out: *mut *mut TfhePolyWeights) -> c_int;
    fn tfhe_poly_weights_destroy(weights: *mut TfhePolyWeights);
    fn tfhe_poly_weights_info(weights: *const TfhePolyWeights, outputs: *mut usize, channels: *mut usize, weight_bits: *mut u32,
                              rows_per_pass: *mut u32) -> c_int;
    fn tfhe_glwe_conv_batch(ctx: *mut TfheContext, x: *const u32, queries: usize, weights: *const TfhePolyWeights,
                            bias: *const u32, out: *mut u32) -> c_int;
    fn tfhe_sample_extract_indices(ctx: *mut TfheContext, glwe: *const u32, batch: usize, indices: *const u32, count: usize,
                                   lwe_out: *mut u32) -> c_int;
    // GLWE key switching and automorphisms (include/tfhe_hip.h)
    fn tfhe_glwe_sk_automorphism(glwe_sk: *const u32, k: usize, log_n: u32, t: usize, out: *mut i32) -> c_int;
    fn tfhe_generate_glwe_switch_key(ctx: *mut TfheContext, from_polys: *const i32, glwe_sk: *const u32, key: *mut u32) -> c_int;
    fn tfhe_prepare_glwe_switch_key(ctx: *mut TfheContext, key: *const u32, out: *mut *mut TfheGlweSwitchKey) -> c_int;
    fn tfhe_glwe_switch_key_destroy(key: *mut TfheGlweSwitchKey);
    fn tfhe_generate_multibit_key(ctx: *mut TfheContext, lwe_sk: *const u32, glwe_sk: *const u32, g: c_uint, bsk_mb: *mut u32) -> c_int;
    fn tfhe_prepare_multibit_key(ctx: *mut TfheContext, bsk_mb: *const u32, g: c_uint, out: *mut *mut TfheMultibitKey) -> c_int;
    fn tfhe_multibit_key_destroy(key: *mut TfheMultibitKey);
    fn tfhe_multibit_bootstrap_batch(ctx: *mut TfheContext, key: *const TfheMultibitKey, lwe_in: *const u32, batch: usize,
                                     test_vector_poly: *const u32, tv_count: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_block_rotate_max_block(ctx: *mut TfheContext, max_block: *mut c_uint) -> c_int;
    fn tfhe_block_bootstrap_batch(ctx: *mut TfheContext, lwe_in: *const u32, batch: usize, block: c_uint,
                                  test_vector_poly: *const u32, tv_count: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_glwe_automorphism_batch(ctx: *mut TfheContext, glwe_in: *const u32, batch: usize, t: usize,
                                    key: *const TfheGlweSwitchKey, add_input: c_int, glwe_out: *mut u32) -> c_int;
    fn tfhe_cmux_batch(ctx: *mut TfheContext, ggsw: *const u32, ggsw_count: usize, ct0: *const u32,
                       ct1: *mut u32, batch: usize, glwe_out: *mut u32) -> c_int;
    fn tfhe_gate_batch(ctx: *mut TfheContext, truth: *const u32, ct0: *const u32, ct1: *const u32,
                       batch: usize, lwe_out: *mut u32) -> c_int;
    fn tfhe_construct_test_from_lut(params: *const CTfheParams, lut: *const u32, lut_len: usize, out: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn tfhe_context_set_stream(ctx: *mut TfheContext, hip_stream: *mut c_void) -> c_int;
    fn tfhe_bootstrapping_key_gen(ctx: *mut TfheContext, lwe_sk: *const u32, glwe_sk: *const u32,
                                  bsk: *mut u32, ksk: *mut u32, load: c_int) -> c_int;
    fn tfhe_lwe_encrypt_batch(ctx: *mut TfheContext, lwe_sk: *const u32, dimension: usize,
                              plaintexts: *const u32, lwe: *mut u32, batch: usize) -> c_int;
    fn tfhe_lwe_decrypt_batch(ctx: *mut TfheContext, lwe_sk: *const u32, dimension: usize,
                              lwe: *const u32, batch: usize, plaintext_out: *mut u32) -> c_int;
}

/// The reference panics on failure (assert!/unwrap); so does this shim -- but only on the Rust
/// side of the boundary: the C ABI itself returns status codes and never unwinds.
fn check(ctx: *const TfheContext, status: c_int, what: &str) {
    if status != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(tfhe_last_error(ctx)) }.to_string_lossy().into_owned();
        panic!("{what}: status {status}: {msg}");
    }
}

fn check_pool(pool: *const TfhePool, status: c_int, what: &str) {
    if status != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(tfhe_pool_last_error(pool)) }.to_string_lossy().into_owned();
        panic!("{what}: status {status}: {msg}");
    }
}

/// Owns the device copies of ONE `BootstrappingKey` (bootstrapping.rs:18-21) on one or several GPUs of a node.
/// `pool` spans the listed devices; `ctx` is its first member (borrowed) and serves the single-ciphertext calls.
pub struct GpuBootstrappingKey { pool: *mut TfhePool, ctx: *mut TfheContext, params: CTfheParams }

/// All GPUs of an 8-GPU node: `&ALL_8_GPUS` as the `devices` argument below; `&[0]` is one GPU.
pub const ALL_8_GPUS: [c_int; 8] = [0, 1, 2, 3, 4, 5, 6, 7];

impl GpuBootstrappingKey {
    fn create(params: &CTfheParams, devices: &[c_int]) -> (*mut TfhePool, *mut TfheContext) {
        let mut pool = std::ptr::null_mut();
        let st = unsafe { tfhe_pool_create(params, devices.as_ptr(), devices.len(), 0 /* TFHE_BACKEND_AUTO */, &mut pool) };
        assert!(st == 0, "tfhe_pool_create: status {st}");
        (pool, unsafe { tfhe_pool_member(pool, 0) })
    }

    /// `lwe_sk_ggsw_enc`: the n `GgswCiphertext.data` arrays ((k+1)l, k+1, N); `ksk`: `KeySwitchingKey.data`;
    /// `devices`: HIP device ordinals.  The key crosses PCIe once and is transformed once; the other devices get
    /// the prepared key over xGMI.
    pub fn upload(params: CTfheParams, devices: &[c_int], lwe_sk_ggsw_enc: &[Array3<u32>], ksk: &Array2<u32>) -> Self {
        let mut flat = Vec::new();
        for g in lwe_sk_ggsw_enc { flat.extend_from_slice(g.as_slice().unwrap()); }
        Self::upload_flat(&params, devices, &flat, ksk.as_slice().unwrap())
    }

    /// The same from already flattened buffers: `bsk` [n][(k+1)l][k+1][N], `ksk` [kN*l_ks][n+1]
    /// (the layout of the on-disk format and of tests/golden/).
    pub fn upload_flat(params: &CTfheParams, devices: &[c_int], bsk: &[u32], ksk: &[u32]) -> Self {
        let (pool, ctx) = Self::create(params, devices);
        check_pool(pool, unsafe { tfhe_pool_load_bootstrapping_key(pool, bsk.as_ptr(), ksk.as_ptr()) }, "load key");
        GpuBootstrappingKey { pool, ctx, params: *params }
    }

    /// Key of the unrolled blind rotation the crate sketches in notes/BMMP Bootstrapping.md:13-25:
    /// `bsk_bmmp` [n/2][3][(k+1)l][k+1][N] = GGSW(s s'), GGSW(s (1-s')), GGSW(s' (1-s)) per pair of key
    /// bits.  `bootstrap` / the gates then consume two key bits per step (N = 512, even n).
    pub fn upload_bmmp_flat(params: &CTfheParams, devices: &[c_int], bsk_bmmp: &[u32], ksk: &[u32]) -> Self {
        let (pool, ctx) = Self::create(params, devices);
        check_pool(pool, unsafe { tfhe_pool_load_bootstrapping_key_bmmp(pool, bsk_bmmp.as_ptr(), ksk.as_ptr()) }, "load BMMP key");
        GpuBootstrappingKey { pool, ctx, params: *params }
    }
}

/// Kernel shape of the blind rotation (`tfhe_context_set_kernel_shape`): `Auto` picks by batch -- a single `bootstrap()`
/// (the crate's own call, bootstrapping.rs:58-65) or a narrow gate level gets the wide team, large batches the throughput
/// kernels; the bits are the same.
#[derive(Clone, Copy)]
pub enum KernelShape { Auto = 0, Wide = 1, Team = 2 }

impl GpuBootstrappingKey {
    pub fn set_kernel_shape(&self, shape: KernelShape) {
        check_pool(self.pool, unsafe { tfhe_pool_set_kernel_shape(self.pool, shape as c_int) }, "set kernel shape");
    }
}

/// Path of `key_switch_lwe` (key_switching.rs:63-103; `tfhe_context_set_key_switch_path`): `Auto` takes the int8 matrix
/// cores over the key prepared at load wherever the key-switch digits fit int8 (log_base <= 6),
/// `Matrix` insists (and panics where they do not fit); the bits are the same.
#[derive(Clone, Copy)]
pub enum KeySwitchPath { Auto = 0, Scalar = 1, Matrix = 2 }

impl GpuBootstrappingKey {
    pub fn set_key_switch_path(&self, path: KeySwitchPath) {
        check_pool(self.pool, unsafe { tfhe_pool_set_key_switch_path(self.pool, path as c_int) }, "set key-switch path");
    }
}

impl Drop for GpuBootstrappingKey {
    fn drop(&mut self) { unsafe { tfhe_pool_destroy(self.pool) } }  // destroys the member contexts too
}

/// bootstrapping.rs:58-65.  `_lwe_secret_key` / `_glwe_secret_key` keep the positional slots of the
/// reference signature; the reference never reads them (bootstrapping.rs:66-120) and neither do we.
pub fn bootstrap<SK1, SK2>(bk: &GpuBootstrappingKey, lwe_ciphertext: &Array1<u32>, _lwe_secret_key: &SK1,
                           _glwe_secret_key: &SK2, test_vector_poly: &Array1<u32>) -> Array1<u32> {
    let mut out = Array1::<u32>::zeros(lwe_ciphertext.len());
    check(bk.ctx, unsafe {
        tfhe_bootstrap_batch(bk.ctx, lwe_ciphertext.as_slice().unwrap().as_ptr(), 1,
                             test_vector_poly.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "bootstrap");
    out
}

/// Batched form: `lwe_ciphertexts` is (batch, n+1) row-major.  Independent bootstraps: the batch is cut into
/// contiguous slices over the devices the key was uploaded to (8 GPUs: batch 2^20 -> 2^17 per GPU); no collective.
pub fn bootstrap_batch(bk: &GpuBootstrappingKey, lwe_ciphertexts: &Array2<u32>, test_vector_poly: &Array1<u32>) -> Array2<u32> {
    let mut out = Array2::<u32>::zeros(lwe_ciphertexts.raw_dim());
    check_pool(bk.pool, unsafe {
        tfhe_pool_bootstrap_batch(bk.pool, lwe_ciphertexts.as_slice().unwrap().as_ptr(), lwe_ciphertexts.nrows(),
                                  test_vector_poly.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "bootstrap_batch");
    out
}

/// A stream of gates with one truth table `truth[(lhs << 1) | rhs]` (boolean.rs:9-53 per row), sharded like
/// bootstrap_batch: `ct0`, `ct1` are (batch, n+1).
pub fn gate_batch(bk: &GpuBootstrappingKey, truth: [u32; 4], ct0: &Array2<u32>, ct1: &Array2<u32>) -> Array2<u32> {
    let mut out = Array2::<u32>::zeros(ct0.raw_dim());
    check_pool(bk.pool, unsafe {
        tfhe_pool_gate_batch(bk.pool, truth.as_ptr(), ct0.as_slice().unwrap().as_ptr(), ct1.as_slice().unwrap().as_ptr(),
                             ct0.nrows(), out.as_slice_mut().unwrap().as_mut_ptr())
    }, "gate_batch");
    out
}

/// key_switching.rs:63-69 (parameters and key come from the uploaded BootstrappingKey)
pub fn key_switch_lwe(bk: &GpuBootstrappingKey, lwe_ciphertext: &Array1<u32>) -> Array1<u32> {
    let mut out = Array1::<u32>::zeros(bk.params.lwe_dimension as usize + 1);
    check(bk.ctx, unsafe { tfhe_key_switch_batch(bk.ctx, lwe_ciphertext.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr()) }, "key_switch_lwe");
    out
}

/// Completes a packing key [from_dimension*l_ks][k+1][N] whose rows the caller pre-filled like zero GLWE encryptions
/// (uniform masks, error in the body): row i*l_ks + l encrypts from_sk[i] * g_l under `glwe_sk` (no reference counterpart).
pub fn generate_packing_key(bk: &GpuBootstrappingKey, from_sk: &Array1<u32>, glwe_sk: &Array2<u32>, samples: &mut Array3<u32>) {
    check(bk.ctx, unsafe {
        tfhe_generate_packing_key(bk.ctx, from_sk.as_slice().unwrap().as_ptr(), from_sk.len(),
                                  glwe_sk.as_slice().unwrap().as_ptr(), samples.as_slice_mut().unwrap().as_mut_ptr())
    }, "generate_packing_key");
}

/// Prepares and keeps a packing key from an LWE key of `from_dimension` bits (independent of the bootstrapping key).
pub fn load_packing_key(bk: &GpuBootstrappingKey, pksk: &Array3<u32>, from_dimension: usize) {
    check(bk.ctx, unsafe { tfhe_load_packing_key(bk.ctx, pksk.as_slice().unwrap().as_ptr(), from_dimension) }, "load_packing_key");
}

/// Up to N LWE ciphertexts (rows of `lwe`, from_dimension+1 words each) -> one GLWE (k+1, N) whose coefficient j
/// decrypts to what row j decrypts to.
pub fn pack_lwe(bk: &GpuBootstrappingKey, lwe: &Array2<u32>) -> Array2<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let mut from_dimension = 0usize;
    check(bk.ctx, unsafe { tfhe_packing_key_dimension(bk.ctx, &mut from_dimension) }, "pack_lwe: no packing key loaded");
    // the ABI reads from_dimension+1 words per ciphertext
    assert!(lwe.ncols() == from_dimension + 1 && lwe.nrows() >= 1 && lwe.nrows() <= n, "pack_lwe: rows of from_dimension+1 words, 1..=N of them");
    let mut out = Array2::<u32>::zeros((bk.params.glwe_dimension as usize + 1, n));
    check(bk.ctx, unsafe {
        tfhe_pack_lwe_batch(bk.ctx, lwe.as_slice().unwrap().as_ptr(), 1, lwe.nrows(), out.as_slice_mut().unwrap().as_mut_ptr())
    }, "pack_lwe");
    out
}

/// Tree over `selectors` (depth, (k+1)l, k+1, N) flattened to Array2 rows -- selector i is address bit i -- and 2^depth
/// leaves (2^depth, k+1, N): the GLWE (k+1, N) of leaf sum_i b_i 2^i (no reference counterpart).
pub fn cmux_tree(bk: &GpuBootstrappingKey, selectors: &Array2<u32>, leaves: &Array3<u32>) -> Array2<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k1 = bk.params.glwe_dimension as usize + 1;
    let depth = selectors.nrows();
    let ggsw = k1 * bk.params.pbs_decomposer.levels as usize * k1 * n;
    // the ABI reads depth GGSWs and 2^depth GLWEs
    assert!(depth >= 1 && depth <= 20 && selectors.ncols() == ggsw, "cmux_tree: depth rows of (k+1) l (k+1) N words, depth 1..=20");
    assert!(leaves.dim() == (1usize << depth, k1, n), "cmux_tree: 2^depth leaves of (k+1, N)");
    let mut out = Array2::<u32>::zeros((k1, n));
    check(bk.ctx, unsafe {
        tfhe_cmux_tree(bk.ctx, selectors.as_slice().unwrap().as_ptr(), 1, depth, leaves.as_slice().unwrap().as_ptr(), 1, 1,
                       out.as_slice_mut().unwrap().as_mut_ptr())
    }, "cmux_tree");
    out
}

/// table[address] for a clear table of 2^depth un-encoded values below 2^log_p and the address bits GGSW-encrypted in
/// `selectors` (as for cmux_tree): an LWE of k N + 1 words under the flattened GLWE key.
pub fn table_lookup(bk: &GpuBootstrappingKey, selectors: &Array2<u32>, table: &Array1<u32>) -> Array1<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k = bk.params.glwe_dimension as usize;
    let depth = selectors.nrows();
    let ggsw = (k + 1) * bk.params.pbs_decomposer.levels as usize * (k + 1) * n;
    assert!(depth >= 1 && depth <= bk.params.glwe_poly_degree as usize + 20 && selectors.ncols() == ggsw,
            "table_lookup: depth rows of (k+1) l (k+1) N words, depth 1..=log2 N + 20");
    assert!(table.len() == 1usize << depth, "table_lookup: 2^depth entries");
    let mut out = Array1::<u32>::zeros(k * n + 1);
    check(bk.ctx, unsafe {
        tfhe_table_lookup(bk.ctx, selectors.as_slice().unwrap().as_ptr(), 1, depth, table.as_slice().unwrap().as_ptr(), 1, 1,
                          out.as_slice_mut().unwrap().as_mut_ptr())
    }, "table_lookup");
    out
}

/// One node of a branching program: cmux(C_sel, R(lo), X^rot R(hi)); a reference below n_terminals names a terminal,
/// any other node `reference - n_terminals`, which must come earlier (tfhe_program_node of include/tfhe_hip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ProgramNode {
    pub sel: u32,
    pub lo: u32,
    pub hi: u32,
    pub rot: u32,
}

/// Evaluate a branching program on the input bits GGSW-encrypted in `selectors` (row s = input s, as for cmux_tree):
/// `terminals` (n_terminals, N) clear message words, `outputs` references.  One LWE of k N + 1 words per output under
/// the flattened GLWE key (no reference counterpart).
pub fn cmux_program(bk: &GpuBootstrappingKey, selectors: &Array2<u32>, nodes: &[ProgramNode], terminals: &Array2<u32>,
                    outputs: &[u32]) -> Array2<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k = bk.params.glwe_dimension as usize;
    let ggsw = (k + 1) * bk.params.pbs_decomposer.levels as usize * (k + 1) * n;
    assert!(selectors.ncols() == ggsw, "cmux_program: one row of (k+1) l (k+1) N words per input");
    assert!(terminals.nrows() >= 1 && terminals.ncols() == n && !outputs.is_empty(), "cmux_program: terminals (n_terminals, N), at least one output");
    let mut out = Array2::<u32>::zeros((outputs.len(), k * n + 1));
    check(bk.ctx, unsafe {
        tfhe_cmux_program(bk.ctx, selectors.as_slice().unwrap().as_ptr(), 1, selectors.nrows(), 1, nodes.as_ptr(), nodes.len(),
                          terminals.as_slice().unwrap().as_ptr(), terminals.nrows(), outputs.as_ptr(), outputs.len(),
                          std::ptr::null_mut(), out.as_slice_mut().unwrap().as_mut_ptr())
    }, "cmux_program");
    out
}

/// Demux over `selectors` (as for cmux_tree) of one GLWE `x` (k+1, N): 2^depth leaves (2^depth, k+1, N), leaf
/// sum_i b_i 2^i carries x and every other one an encryption of 0 (no reference counterpart).
pub fn demux_tree(bk: &GpuBootstrappingKey, selectors: &Array2<u32>, x: &Array2<u32>) -> Array3<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k1 = bk.params.glwe_dimension as usize + 1;
    let depth = selectors.nrows();
    let ggsw = k1 * bk.params.pbs_decomposer.levels as usize * k1 * n;
    assert!(depth >= 1 && depth <= 20 && selectors.ncols() == ggsw, "demux_tree: depth rows of (k+1) l (k+1) N words, depth 1..=20");
    assert!(x.dim() == (k1, n), "demux_tree: one GLWE of (k+1, N)");
    let mut out = Array3::<u32>::zeros((1usize << depth, k1, n));
    check(bk.ctx, unsafe {
        tfhe_demux_tree(bk.ctx, selectors.as_slice().unwrap().as_ptr(), 1, depth, x.as_slice().unwrap().as_ptr(), 1,
                        out.as_slice_mut().unwrap().as_mut_ptr(), 1, 0)
    }, "demux_tree");
    out
}

/// table[address] += value, obliviously: `table` (max(1, 2^depth / N), k+1, N) holds entry a in coefficient a mod N of
/// GLWE a / N and is updated in place; `value` (k+1, N) holds the encoded value in coefficient 0 of its phase.  The
/// write adds: to replace an entry write new - old.
pub fn table_write(bk: &GpuBootstrappingKey, selectors: &Array2<u32>, value: &Array2<u32>, table: &mut Array3<u32>) {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k1 = bk.params.glwe_dimension as usize + 1;
    let depth = selectors.nrows();
    let ggsw = k1 * bk.params.pbs_decomposer.levels as usize * k1 * n;
    let log_n = bk.params.glwe_poly_degree as usize;
    assert!(depth >= 1 && depth <= log_n + 20 && selectors.ncols() == ggsw,
            "table_write: depth rows of (k+1) l (k+1) N words, depth 1..=log2 N + 20");
    let glwes = 1usize << depth.saturating_sub(log_n);
    assert!(value.dim() == (k1, n) && table.dim() == (glwes, k1, n), "table_write: a value (k+1, N) and max(1, 2^depth / N) table GLWEs");
    check(bk.ctx, unsafe {
        tfhe_table_write(bk.ctx, selectors.as_slice().unwrap().as_ptr(), 1, depth, value.as_slice().unwrap().as_ptr(),
                         table.as_slice_mut().unwrap().as_mut_ptr(), 1, 1)
    }, "table_write");
}

/// table[address] of an encrypted table in table_write's layout: an LWE of k N + 1 words under the flattened GLWE key.
pub fn table_lookup_glwe(bk: &GpuBootstrappingKey, selectors: &Array2<u32>, table: &Array3<u32>) -> Array1<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k = bk.params.glwe_dimension as usize;
    let depth = selectors.nrows();
    let ggsw = (k + 1) * bk.params.pbs_decomposer.levels as usize * (k + 1) * n;
    let log_n = bk.params.glwe_poly_degree as usize;
    assert!(depth >= 1 && depth <= log_n + 20 && selectors.ncols() == ggsw,
            "table_lookup_glwe: depth rows of (k+1) l (k+1) N words, depth 1..=log2 N + 20");
    assert!(table.dim() == (1usize << depth.saturating_sub(log_n), k + 1, n), "table_lookup_glwe: max(1, 2^depth / N) table GLWEs");
    let mut out = Array1::<u32>::zeros(k * n + 1);
    check(bk.ctx, unsafe {
        tfhe_table_lookup_glwe(bk.ctx, selectors.as_slice().unwrap().as_ptr(), 1, depth, table.as_slice().unwrap().as_ptr(), 1, 1,
                               out.as_slice_mut().unwrap().as_mut_ptr())
    }, "table_lookup_glwe");
    out
}

/// Blind rotation that starts from the GLWE ciphertext `acc` (k+1, N), words already encoded:
/// X^{-(b~ + rotation_offset)} acc, then the n CMUXes (no reference counterpart).
pub fn blind_rotate_glwe(bk: &GpuBootstrappingKey, lwe: &Array1<u32>, acc: &Array2<u32>, rotation_offset: usize) -> Array2<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k1 = bk.params.glwe_dimension as usize + 1;
    assert!(lwe.len() == bk.params.lwe_dimension as usize + 1 && acc.dim() == (k1, n) && rotation_offset < 2 * n,
            "blind_rotate_glwe: lwe of n+1 words, acc (k+1, N), rotation_offset below 2N");
    let mut out = Array2::<u32>::zeros((k1, n));
    check(bk.ctx, unsafe {
        tfhe_blind_rotate_glwe_batch(bk.ctx, lwe.as_slice().unwrap().as_ptr(), 1, acc.as_slice().unwrap().as_ptr(), 1,
                                     rotation_offset, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "blind_rotate_glwe");
    out
}

/// blind_rotate_glwe + sample extraction at 0 + key switch: with `acc` a GLWE encryption of the encoded test vector,
/// a bootstrap against a table the server cannot read.
pub fn bootstrap_glwe(bk: &GpuBootstrappingKey, lwe: &Array1<u32>, acc: &Array2<u32>, rotation_offset: usize) -> Array1<u32> {
    let n = 1usize << bk.params.glwe_poly_degree;
    let k1 = bk.params.glwe_dimension as usize + 1;
    assert!(lwe.len() == bk.params.lwe_dimension as usize + 1 && acc.dim() == (k1, n) && rotation_offset < 2 * n,
            "bootstrap_glwe: lwe of n+1 words, acc (k+1, N), rotation_offset below 2N");
    let mut out = Array1::<u32>::zeros(lwe.len());
    check(bk.ctx, unsafe {
        tfhe_bootstrap_glwe_batch(bk.ctx, lwe.as_slice().unwrap().as_ptr(), 1, acc.as_slice().unwrap().as_ptr(), 1,
                                  rotation_offset, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "bootstrap_glwe");
    out
}

/// table[sum_t x_t B^t] of the d encrypted digits in the rows of `digits` (d, n+1), B = 2^log_p, digit 0 least
/// significant; `table` holds B^d un-encoded values below B.  Needs a packing key from the flattened GLWE key.
pub fn tree_lut(bk: &GpuBootstrappingKey, digits: &Array2<u32>, table: &Array1<u32>) -> Array1<u32> {
    let d = digits.nrows();
    let log_p = bk.params.log_p as usize;
    let width = bk.params.lwe_dimension as usize + 1;
    assert!(d >= 1 && d * log_p <= 16 && digits.ncols() == width, "tree_lut: d rows of n+1 words, d * log_p in 1..=16");
    assert!(table.len() == 1usize << (d * log_p), "tree_lut: B^d entries");
    let flat = digits.as_slice().unwrap();
    let ptrs: Vec<*const u32> = (0..d).map(|t| flat[t * width..].as_ptr()).collect();
    let mut out = Array1::<u32>::zeros(width);
    check(bk.ctx, unsafe {
        tfhe_tree_lut_batch(bk.ctx, ptrs.as_ptr(), d, 1, table.as_slice().unwrap().as_ptr(), 1, 1,
                            out.as_slice_mut().unwrap().as_mut_ptr())
    }, "tree_lut");
    out
}

/// Digit extraction: `lwe` (batch, n+1) with phase v 2^lsb + e -> (`digits` arrays (digits, batch, n+1) of `digit_bits`
/// bits of v each at `out_lsb`, digit 0 least significant; the remainder (batch, n+1): the input with the extracted bits
/// cleared).  One sign bootstrap per bit (no reference counterpart).  Ciphertexts of n+1 words: the reference's bootstrap
/// order only, like the neighbouring wrappers (the key-switch-first order's k N + 1 words go through the C ABI).
pub fn extract_digits(bk: &GpuBootstrappingKey, lwe: &Array2<u32>, lsb: u32, digit_bits: u32, digits: u32, out_lsb: u32)
                      -> (Array3<u32>, Array2<u32>) {
    let (batch, width) = lwe.dim();
    assert!(width == bk.params.lwe_dimension as usize + 1 && batch >= 1 && digits >= 1 && digits <= 16,
            "extract_digits: ciphertexts of n+1 words, digits in 1..=16");
    let mut out = Array3::<u32>::zeros((digits as usize, batch, width));
    let mut rem = Array2::<u32>::zeros((batch, width));
    let flat = out.as_slice_mut().unwrap();
    let ptrs: Vec<*mut u32> = (0..digits as usize).map(|t| flat[t * batch * width..].as_mut_ptr()).collect();
    check(bk.ctx, unsafe {
        tfhe_extract_digits_batch(bk.ctx, lwe.as_slice().unwrap().as_ptr(), batch, lsb as c_uint, digit_bits as c_uint,
                                  digits as c_uint, out_lsb as c_uint, ptrs.as_ptr(), rem.as_slice_mut().unwrap().as_mut_ptr())
    }, "extract_digits");
    (out, rem)
}

/// Wide LUT: T[v] of the d log_p low bits v of every row of `lwe` (batch, n+1), phase v 2^lsb + e; `table` B^d un-encoded
/// entries -> (batch, n+1).  extract_digits then tree_lut in one call.  The reference's bootstrap order only, as above.
pub fn wide_lut(bk: &GpuBootstrappingKey, lwe: &Array2<u32>, lsb: u32, d: usize, table: &Array1<u32>) -> Array2<u32> {
    let (batch, width) = lwe.dim();
    let log_p = bk.params.log_p as usize;
    assert!(d >= 1 && d * log_p <= 16 && width == bk.params.lwe_dimension as usize + 1, "wide_lut: n+1 words, d * log_p in 1..=16");
    assert!(table.len() == 1usize << (d * log_p), "wide_lut: B^d entries");
    let mut out = Array2::<u32>::zeros((batch, width));
    check(bk.ctx, unsafe {
        tfhe_wide_lut_batch(bk.ctx, lwe.as_slice().unwrap().as_ptr(), batch, lsb as c_uint, d, table.as_slice().unwrap().as_ptr(),
                            1, 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "wide_lut");
    out
}

/// Radix carry propagation: `x` (batch, blocks, n+1), blocks of any value below 2^log_p (log_p = 2 m: m message bits and m
/// carry bits), block 0 least significant -> the clean integers of the same values, in 3 + ceil(log2(blocks - 1)) bootstrap
/// levels (no reference counterpart).  The reference's bootstrap order only, as above.
pub fn radix_propagate(bk: &GpuBootstrappingKey, x: &Array3<u32>) -> Array3<u32> {
    let (batch, blocks, width) = x.dim();
    assert!(width == bk.params.lwe_dimension as usize + 1 && batch >= 1 && blocks >= 1, "radix_propagate: ciphertexts of n+1 words");
    let mut out = Array3::<u32>::zeros((batch, blocks, width));
    check(bk.ctx, unsafe {
        tfhe_radix_propagate_batch(bk.ctx, x.as_slice().unwrap().as_ptr(), batch, blocks, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "radix_propagate");
    out
}

/// One level of table lookups on radix blocks: out[q][j] = tables[table_of_block[j]][wa a[q][j] + wb b[q][j]], `tables`
/// (count, 2^log_p) of un-encoded values; `b` None: a univariate lookup.  The caller keeps wa v_a + wb v_b below 2^log_p.
pub fn radix_map(bk: &GpuBootstrappingKey, a: &Array3<u32>, wa: u32, b: Option<&Array3<u32>>, wb: u32, tables: &Array2<u32>,
                 table_of_block: &Array1<u32>) -> Array3<u32> {
    let (batch, blocks, width) = a.dim();
    let (count, values) = tables.dim();
    assert!(width == bk.params.lwe_dimension as usize + 1 && batch >= 1 && blocks >= 1, "radix_map: ciphertexts of n+1 words");
    assert!(count >= 1 && values == 1usize << bk.params.log_p && table_of_block.len() == blocks, "radix_map: tables of 2^log_p values, one index per block");
    assert!(b.map_or(true, |b| b.dim() == a.dim()), "radix_map: operands of one shape");
    let mut out = Array3::<u32>::zeros((batch, blocks, width));
    check(bk.ctx, unsafe {
        tfhe_radix_map_batch(bk.ctx, a.as_slice().unwrap().as_ptr(), blocks, wa, 0, -1,
                             b.map_or(std::ptr::null(), |b| b.as_slice().unwrap().as_ptr()), blocks, wb, 0, -1, batch, blocks,
                             tables.as_slice().unwrap().as_ptr(), count, table_of_block.as_slice().unwrap().as_ptr(),
                             out.as_slice_mut().unwrap().as_mut_ptr())
    }, "radix_map");
    out
}

/// Radix comparison of clean `a`, `b` (batch, blocks, n+1): predicate 0 eq, 1 ne, 2 lt, 3 le, 4 gt, 5 ge -> (batch, n+1), one
/// block in {0, 1} per row, in 1 + ceil(log2 blocks) bootstrap levels.
pub fn radix_compare(bk: &GpuBootstrappingKey, a: &Array3<u32>, b: &Array3<u32>, predicate: u32) -> Array2<u32> {
    let (batch, blocks, width) = a.dim();
    assert!(width == bk.params.lwe_dimension as usize + 1 && batch >= 1 && blocks >= 1 && b.dim() == a.dim() && predicate <= 5,
            "radix_compare: two integers of one shape, ciphertexts of n+1 words, a predicate in 0..=5");
    let mut out = Array2::<u32>::zeros((batch, width));
    check(bk.ctx, unsafe {
        tfhe_radix_compare_batch(bk.ctx, a.as_slice().unwrap().as_ptr(), b.as_slice().unwrap().as_ptr(), batch, blocks, predicate as c_uint,
                                 out.as_slice_mut().unwrap().as_mut_ptr())
    }, "radix_compare");
    out
}

/// The public seed of a seeded object (tfhe_seed): a 256-bit key and a stream number.  One (key, domain, stream) must never
/// produce the masks of two objects under the same secret key.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct TfheSeed { pub key: [u32; 8], pub stream: u64 }

pub const SEED_DOMAIN_LWE: u32 = 0x3145574c;
pub const SEED_DOMAIN_GLWE: u32 = 0x31574c47;

/// G(seed, domain)[first_word .. first_word + count): the definition of the mask generator (host code, no GPU).
pub fn seed_words(seed: &TfheSeed, domain: u32, first_word: u64, count: usize) -> Array1<u32> {
    let mut out = Array1::<u32>::zeros(count);
    let st = unsafe { tfhe_seed_words(seed, domain, first_word, count, out.as_slice_mut().unwrap().as_mut_ptr()) };
    assert!(st == 0, "seed_words: the word range must stay within 2^36");
    out
}

/// Seeded LWE rows: `bodies` (rows) of rows first_row.. of `seed` -> (rows, dimension + 1).
pub fn expand_lwe_rows(bk: &GpuBootstrappingKey, seed: &TfheSeed, bodies: &Array1<u32>, first_row: u64, dimension: usize) -> Array2<u32> {
    let rows = bodies.len();
    assert!(rows >= 1 && dimension >= 1, "expand_lwe_rows: at least one row and one mask word");
    let mut out = Array2::<u32>::zeros((rows, dimension + 1));
    check(bk.ctx, unsafe {
        tfhe_expand_lwe_rows(bk.ctx, seed, bodies.as_slice().unwrap().as_ptr(), first_row, rows, dimension, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "expand_lwe_rows");
    out
}

/// Seeded GLWE rows: `bodies` (rows, N) of rows first_row.. of `seed` -> (rows, k+1, N).
pub fn expand_glwe_rows(bk: &GpuBootstrappingKey, seed: &TfheSeed, bodies: &Array2<u32>, first_row: u64) -> Array3<u32> {
    let (rows, n) = bodies.dim();
    assert!(rows >= 1 && n == 1usize << bk.params.glwe_poly_degree, "expand_glwe_rows: bodies (rows, N)");
    let mut out = Array3::<u32>::zeros((rows, bk.params.glwe_dimension as usize + 1, n));
    check(bk.ctx, unsafe {
        tfhe_expand_glwe_rows(bk.ctx, seed, bodies.as_slice().unwrap().as_ptr(), first_row, rows, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "expand_glwe_rows");
    out
}

/// The bodies (rows) of full LWE rows (rows, dimension + 1).
pub fn compress_lwe_rows(bk: &GpuBootstrappingKey, lwe: &Array2<u32>) -> Array1<u32> {
    let (rows, width) = lwe.dim();
    assert!(rows >= 1 && width >= 2, "compress_lwe_rows: lwe (rows, dimension + 1)");
    let mut out = Array1::<u32>::zeros(rows);
    check(bk.ctx, unsafe {
        tfhe_compress_lwe_rows(bk.ctx, lwe.as_slice().unwrap().as_ptr(), rows, width - 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "compress_lwe_rows");
    out
}

/// The body polynomials (rows, N) of full GLWE rows (rows, k+1, N).
pub fn compress_glwe_rows(bk: &GpuBootstrappingKey, glwe: &Array3<u32>) -> Array2<u32> {
    let (rows, polys, n) = glwe.dim();
    assert!(rows >= 1 && polys == bk.params.glwe_dimension as usize + 1 && n == 1usize << bk.params.glwe_poly_degree, "compress_glwe_rows: glwe (rows, k+1, N)");
    let mut out = Array2::<u32>::zeros((rows, n));
    check(bk.ctx, unsafe {
        tfhe_compress_glwe_rows(bk.ctx, glwe.as_slice().unwrap().as_ptr(), rows, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "compress_glwe_rows");
    out
}

/// Replace the loaded key by its seeded form: bsk bodies (n (k+1) l, N) under `bsk_seed`, ksk bodies (kN l_ks) of dimension n
/// under `ksk_seed`; the masks are expanded on the device.
pub fn load_bootstrapping_key_seeded(bk: &GpuBootstrappingKey, bsk_seed: &TfheSeed, bsk_bodies: &Array2<u32>, ksk_seed: &TfheSeed,
                                     ksk_bodies: &Array1<u32>) {
    let p = &bk.params;
    let n = 1usize << p.glwe_poly_degree;
    assert!(bsk_bodies.dim() == (p.lwe_dimension as usize * (p.glwe_dimension as usize + 1) * p.pbs_decomposer.levels as usize, n)
            && ksk_bodies.len() == p.glwe_dimension as usize * n * p.ks_decomposer.levels as usize,
            "load_bootstrapping_key_seeded: bsk bodies (n (k+1) l, N), ksk bodies (kN l_ks)");
    check(bk.ctx, unsafe {
        tfhe_load_bootstrapping_key_seeded(bk.ctx, bsk_seed, bsk_bodies.as_slice().unwrap().as_ptr(), ksk_seed, ksk_bodies.as_slice().unwrap().as_ptr())
    }, "load_bootstrapping_key_seeded");
}

/// bootstrap_batch on seeded inputs: `bodies` (batch) are rows first_row.. of `seed` at dimension n.
pub fn bootstrap_batch_seeded(bk: &GpuBootstrappingKey, seed: &TfheSeed, first_row: u64, bodies: &Array1<u32>,
                              test_vector_poly: &Array1<u32>) -> Array2<u32> {
    let batch = bodies.len();
    assert!(batch >= 1 && test_vector_poly.len() == 1usize << bk.params.glwe_poly_degree, "bootstrap_batch_seeded: one test vector (N)");
    let mut out = Array2::<u32>::zeros((batch, bk.params.lwe_dimension as usize + 1));
    check(bk.ctx, unsafe {
        tfhe_bootstrap_batch_seeded(bk.ctx, seed, first_row, bodies.as_slice().unwrap().as_ptr(), batch,
                                    test_vector_poly.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "bootstrap_batch_seeded");
    out
}

/// Multi-value bootstrap: every table of `luts` (tables, B) of un-encoded values of every row of `lwe` (batch, n+1), from ONE
/// blind rotation per row -> (batch, tables, n+1) (no reference counterpart).  The reference's bootstrap order only, as above.
pub fn multi_value_bootstrap(bk: &GpuBootstrappingKey, lwe: &Array2<u32>, luts: &Array2<u32>) -> Array3<u32> {
    let (batch, width) = lwe.dim();
    let (tables, values) = luts.dim();
    assert!(width == bk.params.lwe_dimension as usize + 1 && batch >= 1, "multi_value_bootstrap: ciphertexts of n+1 words");
    assert!(tables >= 1 && values == 1usize << bk.params.log_p, "multi_value_bootstrap: tables of B = 2^log_p values");
    let mut out = Array3::<u32>::zeros((batch, tables, width));
    check(bk.ctx, unsafe {
        tfhe_multi_value_bootstrap_batch(bk.ctx, lwe.as_slice().unwrap().as_ptr(), batch, luts.as_slice().unwrap().as_ptr(), 1, tables,
                                         out.as_slice_mut().unwrap().as_mut_ptr())
    }, "multi_value_bootstrap");
    out
}

/// The LWE ciphertexts of coefficient 0 of (sum_m coeffs[t][m] X^positions[m]) * glwe[q]: `glwe` (batch, k+1, N), `positions`
/// distinct and below N, `coeffs` (tables, terms) -> (batch, tables, k N + 1), wrapping (no reference counterpart).
pub fn glwe_sparse_extract(bk: &GpuBootstrappingKey, glwe: &Array3<u32>, positions: &Array1<u32>, coeffs: &Array2<i32>) -> Array3<u32> {
    let (batch, polys, n) = glwe.dim();
    let (tables, terms) = coeffs.dim();
    assert!(polys == bk.params.glwe_dimension as usize + 1 && n == 1usize << bk.params.glwe_poly_degree, "glwe_sparse_extract: glwe (batch, k+1, N)");
    assert!(terms == positions.len() && terms >= 1 && tables >= 1, "glwe_sparse_extract: one coefficient per position");
    let mut out = Array3::<u32>::zeros((batch, tables, (polys - 1) * n + 1));
    check(bk.ctx, unsafe {
        tfhe_glwe_sparse_extract_batch(bk.ctx, glwe.as_slice().unwrap().as_ptr(), batch, positions.as_slice().unwrap().as_ptr(), terms,
                                       coeffs.as_slice().unwrap().as_ptr(), 1, tables, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "glwe_sparse_extract");
    out
}

/// Dense(W, bias; x): `x` (queries, I, words), `weights` (O, I), `bias` O already ENCODED words ->
/// (queries, O, words), out[q][o] = sum_i W[o][i] x[q][i] wrapping, bias[o] added to the body (no reference counterpart).
pub fn dense(bk: &GpuBootstrappingKey, x: &Array3<u32>, weights: &Array2<i32>, bias: Option<&Array1<u32>>) -> Array3<u32> {
    let (queries, inputs, words) = x.dim();
    let outputs = weights.nrows();
    assert!(weights.ncols() == inputs && bias.map_or(true, |b| b.len() == outputs), "dense: weights (O, I), bias O words");
    let mut out = Array3::<u32>::zeros((queries, outputs, words));
    check(bk.ctx, unsafe {
        tfhe_lwe_dense_batch(bk.ctx, x.as_slice().unwrap().as_ptr(), queries, inputs, weights.as_slice().unwrap().as_ptr(),
                             bias.map_or(std::ptr::null(), |b| b.as_slice().unwrap().as_ptr()), outputs, words,
                             out.as_slice_mut().unwrap().as_mut_ptr())
    }, "dense");
    out
}

/// A whole layer: out[q][o] = bootstrap(dense(x)[q][o]; test vector o mod tv_count); `test_vectors` (1 or O, N)
/// un-encoded, ciphertexts of n+1 words.
pub fn dense_bootstrap(bk: &GpuBootstrappingKey, x: &Array3<u32>, weights: &Array2<i32>, bias: Option<&Array1<u32>>,
                       test_vectors: &Array2<u32>) -> Array3<u32> {
    let (queries, inputs, words) = x.dim();
    let outputs = weights.nrows();
    let n = 1usize << bk.params.glwe_poly_degree;
    assert!(weights.ncols() == inputs && bias.map_or(true, |b| b.len() == outputs), "dense_bootstrap: weights (O, I), bias O words");
    assert!(words == bk.params.lwe_dimension as usize + 1 && test_vectors.ncols() == n
            && (test_vectors.nrows() == 1 || test_vectors.nrows() == outputs),
            "dense_bootstrap: ciphertexts of n+1 words, 1 or O test vectors of N words");
    let mut out = Array3::<u32>::zeros((queries, outputs, words));
    check(bk.ctx, unsafe {
        tfhe_dense_bootstrap_batch(bk.ctx, x.as_slice().unwrap().as_ptr(), queries, inputs, weights.as_slice().unwrap().as_ptr(),
                                   bias.map_or(std::ptr::null(), |b| b.as_slice().unwrap().as_ptr()), outputs,
                                   test_vectors.as_slice().unwrap().as_ptr(), test_vectors.nrows(),
                                   out.as_slice_mut().unwrap().as_mut_ptr())
    }, "dense_bootstrap");
    out
}

/// A prepared set of clear weight polynomials `weights` (O, C, N) for `glwe_conv` (no reference counterpart); panics with
/// the backend's reason where it admits no pass at their magnitude.  Released on drop.
pub struct PolyWeights { raw: *mut TfhePolyWeights, pub outputs: usize, pub channels: usize, pub weight_bits: u32, pub rows_per_pass: u32 }

impl PolyWeights {
    pub fn new(bk: &GpuBootstrappingKey, weights: &Array3<i32>) -> Self {
        let (outputs, channels, n) = weights.dim();
        assert!(n == 1usize << bk.params.glwe_poly_degree, "PolyWeights: weights (O, C, N)");
        let mut raw = std::ptr::null_mut();
        check(bk.ctx, unsafe {
            tfhe_prepare_poly_weights(bk.ctx, weights.as_slice().unwrap().as_ptr(), outputs, channels, &mut raw)
        }, "prepare_poly_weights");
        let (mut o, mut c, mut bits, mut rows) = (0usize, 0usize, 0u32, 0u32);
        let st = unsafe { tfhe_poly_weights_info(raw, &mut o, &mut c, &mut bits, &mut rows) };
        assert!(st == 0, "tfhe_poly_weights_info: status {st}");
        PolyWeights { raw, outputs: o, channels: c, weight_bits: bits, rows_per_pass: rows }
    }
}

impl Drop for PolyWeights {
    fn drop(&mut self) {
        unsafe { tfhe_poly_weights_destroy(self.raw) };
    }
}

/// Conv(W, bias; x): `x` (queries * C, k+1, N) with the C channels of a query in a row, `bias` (O, N) already ENCODED words
/// -> (queries * O, k+1, N), out[q][o] = sum_c W[o][c](X) * x[q][c] negacyclic and wrapping, bias[o] added to the body.
pub fn glwe_conv(bk: &GpuBootstrappingKey, x: &Array3<u32>, weights: &PolyWeights, bias: Option<&Array2<u32>>) -> Array3<u32> {
    let (rows, polys, n) = x.dim();
    assert!(rows % weights.channels == 0 && polys == bk.params.glwe_dimension as usize + 1 && n == 1usize << bk.params.glwe_poly_degree
            && bias.map_or(true, |b| b.dim() == (weights.outputs, n)), "glwe_conv: x (queries * C, k+1, N), bias (O, N)");
    let queries = rows / weights.channels;
    let mut out = Array3::<u32>::zeros((queries * weights.outputs, polys, n));
    check(bk.ctx, unsafe {
        tfhe_glwe_conv_batch(bk.ctx, x.as_slice().unwrap().as_ptr(), queries, weights.raw,
                             bias.map_or(std::ptr::null(), |b| b.as_slice().unwrap().as_ptr()), out.as_slice_mut().unwrap().as_mut_ptr())
    }, "glwe_conv");
    out
}

/// sample_extract of every GLWE of `glwe` (batch, k+1, N) at every index of `indices` (each below N) -> (batch, count, kN+1)
pub fn sample_extract_indices(bk: &GpuBootstrappingKey, glwe: &Array3<u32>, indices: &Array1<u32>) -> Array3<u32> {
    let (batch, polys, n) = glwe.dim();
    assert!(polys == bk.params.glwe_dimension as usize + 1 && n == 1usize << bk.params.glwe_poly_degree, "sample_extract_indices: glwe (batch, k+1, N)");
    let mut out = Array3::<u32>::zeros((batch, indices.len(), (polys - 1) * n + 1));
    check(bk.ctx, unsafe {
        tfhe_sample_extract_indices(bk.ctx, glwe.as_slice().unwrap().as_ptr(), batch, indices.as_slice().unwrap().as_ptr(), indices.len(),
                                    out.as_slice_mut().unwrap().as_mut_ptr())
    }, "sample_extract_indices");
    out
}

/// sigma_t of a binary GLWE key (k, N) -> (k, N) with entries in {-1, 0, 1}: the `from_polys` of the automorphism key for t
pub fn glwe_sk_automorphism(glwe_sk: &Array2<u32>, t: usize) -> Array2<i32> {
    let (k, n) = glwe_sk.dim();
    assert!(n.is_power_of_two(), "glwe_sk_automorphism: glwe_sk (k, N)");
    let mut out = Array2::<i32>::zeros((k, n));
    let st = unsafe {
        tfhe_glwe_sk_automorphism(glwe_sk.as_slice().unwrap().as_ptr(), k, n.trailing_zeros(), t, out.as_slice_mut().unwrap().as_mut_ptr())
    };
    assert!(st == 0, "glwe_sk_automorphism: a binary key and an odd t in [1, 2N) expected (status {st})");
    out
}

/// A prepared GLWE switch key (no reference counterpart): `samples` (k * l_ks, k+1, N) pre-filled row by row like
/// encrypt_glwe_zero (uniform masks, errors in the body) are completed for `from_polys` (k, N), entries in {-1, 0, 1},
/// and `glwe_sk` (k, N), then prepared on the device; panics with the backend's reason where it refuses a packing key.
/// Released on drop, before the key it was made with.
pub struct GlweSwitchKey { raw: *mut TfheGlweSwitchKey }

impl GlweSwitchKey {
    pub fn new(bk: &GpuBootstrappingKey, from_polys: &Array2<i32>, glwe_sk: &Array2<u32>, samples: &Array3<u32>) -> Self {
        let (k, n) = (bk.params.glwe_dimension as usize, 1usize << bk.params.glwe_poly_degree);
        assert!(from_polys.dim() == (k, n) && glwe_sk.dim() == (k, n)
                && samples.dim() == (k * bk.params.ks_decomposer.levels as usize, k + 1, n),
                "GlweSwitchKey: from_polys (k, N), glwe_sk (k, N), samples (k * l_ks, k+1, N)");
        let mut key = samples.clone();
        check(bk.ctx, unsafe {
            tfhe_generate_glwe_switch_key(bk.ctx, from_polys.as_slice().unwrap().as_ptr(), glwe_sk.as_slice().unwrap().as_ptr(),
                                          key.as_slice_mut().unwrap().as_mut_ptr())
        }, "generate_glwe_switch_key");
        let mut raw = std::ptr::null_mut();
        check(bk.ctx, unsafe { tfhe_prepare_glwe_switch_key(bk.ctx, key.as_slice().unwrap().as_ptr(), &mut raw) },
              "prepare_glwe_switch_key");
        GlweSwitchKey { raw }
    }
}

impl Drop for GlweSwitchKey {
    fn drop(&mut self) {
        unsafe { tfhe_glwe_switch_key_destroy(self.raw) };
    }
}

/// Auto_t(glwe; key) (+ glwe with `add_input`) for every ciphertext of `glwe` (batch, k+1, N): X -> X^t and the switch back
/// to the context's key in one launch; t odd and below 2N
pub fn glwe_automorphism(bk: &GpuBootstrappingKey, glwe: &Array3<u32>, t: usize, key: &GlweSwitchKey, add_input: bool) -> Array3<u32> {
    let (batch, polys, n) = glwe.dim();
    assert!(polys == bk.params.glwe_dimension as usize + 1 && n == 1usize << bk.params.glwe_poly_degree, "glwe_automorphism: glwe (batch, k+1, N)");
    let mut out = Array3::<u32>::zeros((batch, polys, n));
    check(bk.ctx, unsafe {
        tfhe_glwe_automorphism_batch(bk.ctx, glwe.as_slice().unwrap().as_ptr(), batch, t, key.raw, add_input as c_int,
                                     out.as_slice_mut().unwrap().as_mut_ptr())
    }, "glwe_automorphism");
    out
}

/// the plain GLWE key switch (t = 1): from the key's source key to the context's
pub fn glwe_key_switch(bk: &GpuBootstrappingKey, glwe: &Array3<u32>, key: &GlweSwitchKey) -> Array3<u32> {
    glwe_automorphism(bk, glwe, 1, key, false)
}

/// A prepared multi-bit bootstrapping key (no reference counterpart), g in {2, 3, 4} key bits per step: `samples`
/// [ceil(n/g) * (2^g - 1) * (k+1) l][k+1][N], pre-filled like a batch of GGSWs (uniform masks, errors in the body), are
/// completed for `lwe_sk` (n) and `glwe_sk` (k, N), then handed to the device; panics with the reason where the wide team
/// is not offered.  Released on drop, before the key it was made with.
pub struct MultibitKey { raw: *mut TfheMultibitKey }

impl MultibitKey {
    pub fn new(bk: &GpuBootstrappingKey, lwe_sk: &Array1<u32>, glwe_sk: &Array2<u32>, g: u32, samples: &Array3<u32>) -> Self {
        let (k, n) = (bk.params.glwe_dimension as usize, 1usize << bk.params.glwe_poly_degree);
        let dim = bk.params.lwe_dimension as usize;
        assert!((2..=4).contains(&g), "MultibitKey: g must be 2, 3 or 4");
        let rows = ((dim + g as usize - 1) / g as usize) * ((1usize << g) - 1) * (k + 1) * bk.params.pbs_decomposer.levels as usize;
        assert!(lwe_sk.len() == dim && glwe_sk.dim() == (k, n) && samples.dim() == (rows, k + 1, n),
                "MultibitKey: lwe_sk (n), glwe_sk (k, N), samples (ceil(n/g) * (2^g - 1) * (k+1) l, k+1, N)");
        let mut key = samples.clone();
        check(bk.ctx, unsafe {
            tfhe_generate_multibit_key(bk.ctx, lwe_sk.as_slice().unwrap().as_ptr(), glwe_sk.as_slice().unwrap().as_ptr(), g as c_uint,
                                       key.as_slice_mut().unwrap().as_mut_ptr())
        }, "generate_multibit_key");
        let mut raw = std::ptr::null_mut();
        check(bk.ctx, unsafe { tfhe_prepare_multibit_key(bk.ctx, key.as_slice().unwrap().as_ptr(), g as c_uint, &mut raw) },
              "prepare_multibit_key");
        MultibitKey { raw }
    }
}

impl Drop for MultibitKey {
    fn drop(&mut self) {
        unsafe { tfhe_multibit_key_destroy(self.raw) };
    }
}

/// the multi-bit bootstrap of every ciphertext of `lwe_ciphertexts` (batch, boundary dimension + 1) against one clear test
/// vector: the plaintexts of `bootstrap_batch`, other ciphertext bits
pub fn multibit_bootstrap_batch(bk: &GpuBootstrappingKey, key: &MultibitKey, lwe_ciphertexts: &Array2<u32>, test_vector_poly: &Array1<u32>) -> Array2<u32> {
    assert!(test_vector_poly.len() == 1usize << bk.params.glwe_poly_degree, "multibit_bootstrap_batch: test vector (N)");
    let mut out = Array2::<u32>::zeros(lwe_ciphertexts.raw_dim());
    check(bk.ctx, unsafe {
        tfhe_multibit_bootstrap_batch(bk.ctx, key.raw, lwe_ciphertexts.as_slice().unwrap().as_ptr(), lwe_ciphertexts.nrows(),
                                      test_vector_poly.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "multibit_bootstrap_batch");
    out
}

/// The largest block the exactness rule admits for the block-binary blind rotation on this key's context (tfhe_hip.h).
pub fn block_rotate_max_block(bk: &GpuBootstrappingKey) -> u32 {
    let mut b: c_uint = 0;
    check(bk.ctx, unsafe { tfhe_block_rotate_max_block(bk.ctx, &mut b) }, "block_rotate_max_block");
    b as u32
}

/// The block-binary bootstrap (tfhe_hip.h, "block-binary blind rotation"): `block` key bits per decomposition on the loaded,
/// ordinary key -- for LWE secrets with at most one 1 per block of `block` consecutive bits.  One shared test vector (N).
pub fn block_bootstrap_batch(bk: &GpuBootstrappingKey, lwe_ciphertexts: &Array2<u32>, block: u32, test_vector_poly: &Array1<u32>) -> Array2<u32> {
    assert!(test_vector_poly.len() == 1usize << bk.params.glwe_poly_degree, "block_bootstrap_batch: test vector (N)");
    let mut out = Array2::<u32>::zeros(lwe_ciphertexts.raw_dim());
    check(bk.ctx, unsafe {
        tfhe_block_bootstrap_batch(bk.ctx, lwe_ciphertexts.as_slice().unwrap().as_ptr(), lwe_ciphertexts.nrows(), block as c_uint,
                                   test_vector_poly.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "block_bootstrap_batch");
    out
}

/// ggsw.rs:132-136
pub fn external_product(bk: &GpuBootstrappingKey, ggsw_ciphertext: &Array3<u32>, glwe_ciphertext: &Array2<u32>) -> Array2<u32> {
    let mut out = Array2::<u32>::zeros(glwe_ciphertext.raw_dim());
    check(bk.ctx, unsafe {
        tfhe_external_product_batch(bk.ctx, ggsw_ciphertext.as_slice().unwrap().as_ptr(), 1,
                                    glwe_ciphertext.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "external_product");
    out
}

/// ggsw.rs:164-169: `glwe_ciphertext1` is clobbered with ct1 - ct0, as in the reference.
pub fn cmux(bk: &GpuBootstrappingKey, ggsw_ciphertext: &Array3<u32>, glwe_ciphertext0: &Array2<u32>, glwe_ciphertext1: &mut Array2<u32>) -> Array2<u32> {
    let mut out = Array2::<u32>::zeros(glwe_ciphertext0.raw_dim());
    check(bk.ctx, unsafe {
        tfhe_cmux_batch(bk.ctx, ggsw_ciphertext.as_slice().unwrap().as_ptr(), 1, glwe_ciphertext0.as_slice().unwrap().as_ptr(),
                        glwe_ciphertext1.as_slice_mut().unwrap().as_mut_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr())
    }, "cmux");
    out
}

fn gate(bk: &GpuBootstrappingKey, truth: [u32; 4], ct0: &Array1<u32>, ct1: &Array1<u32>) -> Array1<u32> {
    let mut out = Array1::<u32>::zeros(ct0.len());
    check(bk.ctx, unsafe { tfhe_gate_batch(bk.ctx, truth.as_ptr(), ct0.as_slice().unwrap().as_ptr(), ct1.as_slice().unwrap().as_ptr(), 1, out.as_slice_mut().unwrap().as_mut_ptr()) }, "gate");
    out
}
/// boolean.rs:9-14
pub fn and(bk: &GpuBootstrappingKey, ct0: &Array1<u32>, ct1: &Array1<u32>) -> Array1<u32> { gate(bk, [0, 0, 0, 1], ct0, ct1) }
/// boolean.rs:32-37
pub fn or(bk: &GpuBootstrappingKey, ct0: &Array1<u32>, ct1: &Array1<u32>) -> Array1<u32> { gate(bk, [0, 1, 1, 1], ct0, ct1) }
/// not in the reference; built through its closure hook construct_test_vector_boolean (test_vector.rs:5)
pub fn nand(bk: &GpuBootstrappingKey, ct0: &Array1<u32>, ct1: &Array1<u32>) -> Array1<u32> { gate(bk, [1, 1, 1, 0], ct0, ct1) }

/// test_vector.rs:38
pub fn construct_test_from_lut(params: &CTfheParams, lut: &[u32]) -> Array1<u32> {
    let mut out = Array1::<u32>::zeros(1usize << params.glwe_poly_degree);
    let st = unsafe { tfhe_construct_test_from_lut(params, lut.as_ptr(), lut.len(), out.as_slice_mut().unwrap().as_mut_ptr()) };
    assert!(st == 0, "lut must hold 2^log_p entries (test_vector.rs:41)");
    out
}

/// bootstrapping_key_gen (bootstrapping.rs:23-28) on the GPU.  The crate keeps drawing the
/// randomness with its own `rng` -- `bsk_samples` ((n, (k+1)l, k+1, N): `sample_uniform_array`
/// masks, `sample_gaussian_array` errors in every body row, glwe.rs:195,200) and `ksk_samples`
/// ((kN*l_ks, n+1): masks + the error in the b slot, lwe.rs:122-126) -- and the engine turns the
/// buffers into the key in place and installs it.
pub fn bootstrapping_key_gen(params: CTfheParams, lwe_secret_key: &Array1<u32>, glwe_secret_key: &Array2<u32>,
                             mut bsk_samples: ndarray::Array4<u32>, mut ksk_samples: Array2<u32>)
                             -> (GpuBootstrappingKey, ndarray::Array4<u32>, Array2<u32>) {
    // key generation runs on one GPU; upload_flat() the returned arrays to spread the key over more
    let (pool, ctx) = GpuBootstrappingKey::create(&params, &[0]);
    check(ctx, unsafe {
        tfhe_bootstrapping_key_gen(ctx, lwe_secret_key.as_slice().unwrap().as_ptr(),
                                   glwe_secret_key.as_slice().unwrap().as_ptr(),
                                   bsk_samples.as_slice_mut().unwrap().as_mut_ptr(),
                                   ksk_samples.as_slice_mut().unwrap().as_mut_ptr(), 1)
    }, "bootstrapping_key_gen");
    (GpuBootstrappingKey { pool, ctx, params }, bsk_samples, ksk_samples)
}

/// encrypt_lwe_plaintext (lwe.rs:138-160) over a batch: `samples` (batch, n+1) holds the uniform
/// masks and, in the b slot, the error; `plaintexts` are encoded (lwe.rs:81-92).
pub fn encrypt_lwe_batch(bk: &GpuBootstrappingKey, sk: &Array1<u32>, plaintexts: &Array1<u32>, mut samples: Array2<u32>) -> Array2<u32> {
    let batch = samples.nrows();
    check(bk.ctx, unsafe {
        tfhe_lwe_encrypt_batch(bk.ctx, sk.as_slice().unwrap().as_ptr(), sk.len(), plaintexts.as_slice().unwrap().as_ptr(),
                               samples.as_slice_mut().unwrap().as_mut_ptr(), batch)
    }, "encrypt_lwe_batch");
    samples
}

/// decrypt_lwe (lwe.rs:162-173) over a batch -> encoded plaintexts
pub fn decrypt_lwe_batch(bk: &GpuBootstrappingKey, sk: &Array1<u32>, cts: &Array2<u32>) -> Array1<u32> {
    let mut out = Array1::<u32>::zeros(cts.nrows());
    check(bk.ctx, unsafe {
        tfhe_lwe_decrypt_batch(bk.ctx, sk.as_slice().unwrap().as_ptr(), sk.len(), cts.as_slice().unwrap().as_ptr(),
                               cts.nrows(), out.as_slice_mut().unwrap().as_mut_ptr())
    }, "decrypt_lwe_batch");
    out
}
