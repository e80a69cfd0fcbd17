"""Discretised neural networks for Context.dense_bootstrap (include/tfhe_hip.h states the operations): layers of a clear
integer matrix over encrypted messages, one programmable bootstrap per neuron as the activation -- the shape of
FHE-DiNN (Bourse, Minelli, Minihold, Paillier 2018).

  net = Network([Dense(W1, b1, lut1), Dense(W2, b2, lut2)])
  net.check(params, (0, 1))                  # raises unless every pre-activation provably stays in [0, 2^log_p)
  net.evaluate_clear(x)                      # integers in, integers out
  net.run(ctx, cts)                          # ciphertexts [queries][I][io_dim + 1] in and out, one call per layer

A neuron computes lut[sum_i W[o][i] x_i + bias[o]]: messages are integers in [0, 2^log_p), the bias is an integer in
message units (run() encodes it), lut has 2^log_p entries below 2^log_p -- one table for the layer or one per neuron.
A pre-activation outside [0, 2^log_p) would reach into the padding bit, where the bootstrap negates (test_vector.rs:
38-67): check() refuses such a layer instead of evaluating it modulo anything.

The padding bit between layers.  The reference's test vector answers a pre-activation of 0 under a NEGATIVE phase error
with encode(T) - 2^31 instead of encode(T), T = lut[0] (its first half box holds 2^log_p - T, which the negacyclic
rotation negates; nothing of the kind happens where T = 0).  That decodes to T, but an odd weight of the next layer
carries the 2^31 into the next pre-activation's padding bit, where the bootstrap negates.  So check() also requires of
every neuron that feeds another layer: lut[0] = 0, or a pre-activation that provably stays above 0, or only even
weights on it in the next layer.

Only evaluate_clear, check and noise_bound are pure numpy; run() is the only function that touches the device.
"""
from __future__ import annotations

import math

import numpy as np


class Dense:
    def __init__(self, weights, bias=None, lut=None):
        w = np.asarray(weights)
        if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer):
            raise ValueError("weights: a non-empty integer matrix [outputs][inputs] expected")
        if int(w.max()) >= 1 << 31 or int(w.min()) < -(1 << 31):
            raise ValueError("weights must fit int32")
        self.weights = np.ascontiguousarray(w, dtype=np.int32)
        b = np.zeros(w.shape[0], dtype=np.int64) if bias is None else np.asarray(bias, dtype=np.int64).reshape(-1)
        if b.shape != (w.shape[0],):
            raise ValueError(f"bias: {w.shape[0]} integers expected")
        self.bias = b
        if lut is None:
            raise ValueError("lut: the activation's table (2^log_p entries, or one such row per output) is required")
        t = np.asarray(lut, dtype=np.int64)
        if t.ndim not in (1, 2) or (t.ndim == 2 and t.shape[0] != w.shape[0]) or t.shape[-1] < 2 or t.shape[-1] & (t.shape[-1] - 1):
            raise ValueError("lut: 2^log_p entries, or [outputs][2^log_p]")
        if int(t.min()) < 0 or int(t.max()) >= t.shape[-1]:
            raise ValueError("lut entries must be messages: in [0, 2^log_p)")
        self.lut = t

    @property
    def inputs(self) -> int:
        return int(self.weights.shape[1])

    @property
    def outputs(self) -> int:
        return int(self.weights.shape[0])

    def luts(self) -> np.ndarray:
        """[outputs][2^log_p]: the shared table repeated, or the per-neuron tables"""
        return self.lut if self.lut.ndim == 2 else np.broadcast_to(self.lut, (self.outputs, self.lut.size))

    def pre_activations(self, x) -> np.ndarray:
        """x [..][inputs] integers -> W x + bias [..][outputs], unbounded integers"""
        return np.asarray(x, dtype=np.int64) @ self.weights.astype(np.int64).T + self.bias

    def pre_activation_range(self, lo, hi):
        """interval arithmetic: inputs in [lo[i], hi[i]] -> (min, max) [outputs] of the pre-activations"""
        w = self.weights.astype(np.int64)
        lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.int64), (self.inputs,)) for v in (lo, hi))
        pos, neg = np.maximum(w, 0), np.minimum(w, 0)
        return pos @ lo + neg @ hi + self.bias, pos @ hi + neg @ lo + self.bias

    def squared_norms(self) -> np.ndarray:
        """the squared Euclidean norm of every row: what a row multiplies the input noise's variance by"""
        return (self.weights.astype(np.float64) ** 2).sum(axis=1)


class Conv2d:
    """A convolution layer over PACKED images (include/tfhe_hip.h, "encrypted convolutions"): channel c of a query is ONE
    GLWE whose coefficient y W + x carries pixel (y, x) of an H x W image, H W <= N.  The layer is the "valid"
    cross-correlation  pre[o][y][x] = sum_{c,dy,dx} kernels[o][c][dy][dx] image[c][y+dy][x+dx] + bias[o]  followed by the
    table: no stride, no padding, no pooling.

    Tap (dy, dx) sits at coefficient (kh-1-dy) W + (kw-1-dx) of the weight polynomial, so the product carries output
    (y, x) at coefficient (y+kh-1) W + (x+kw-1): the negacyclic wrap and the bleed from one image row into the next land
    only in rows < kh-1 and columns < kw-1, which are never read.  run() extracts the read coefficients and bootstraps
    each one, and returns LWE ciphertexts in (o, y, x) order: the inputs of a Network."""

    def __init__(self, kernels, bias=None, lut=None, image=None):
        w = np.asarray(kernels)
        if w.ndim != 4 or w.size == 0 or not np.issubdtype(w.dtype, np.integer):
            raise ValueError("kernels: a non-empty integer array [outputs][channels][kh][kw] expected")
        if int(w.max()) >= 1 << 31 or int(w.min()) < -(1 << 31):
            raise ValueError("kernels must fit int32")
        if image is None or len(image) != 2 or int(image[0]) < w.shape[2] or int(image[1]) < w.shape[3]:
            raise ValueError("image: (H, W), at least as large as the kernel, is required")
        self.kernels = np.ascontiguousarray(w, dtype=np.int32)
        self.image = (int(image[0]), int(image[1]))
        b = np.zeros(w.shape[0], dtype=np.int64) if bias is None else np.asarray(bias, dtype=np.int64).reshape(-1)
        if b.shape != (w.shape[0],):
            raise ValueError(f"bias: {w.shape[0]} integers expected")
        self.bias = b
        if lut is None:
            raise ValueError("lut: the activation's table (2^log_p entries, or one such row per output) is required")
        t = np.asarray(lut, dtype=np.int64)
        if t.ndim not in (1, 2) or (t.ndim == 2 and t.shape[0] != w.shape[0]) or t.shape[-1] < 2 or t.shape[-1] & (t.shape[-1] - 1):
            raise ValueError("lut: 2^log_p entries, or [outputs][2^log_p]")
        if int(t.min()) < 0 or int(t.max()) >= t.shape[-1]:
            raise ValueError("lut entries must be messages: in [0, 2^log_p)")
        self.lut = t

    @property
    def outputs(self) -> int:
        return int(self.kernels.shape[0])

    @property
    def channels(self) -> int:
        return int(self.kernels.shape[1])

    @property
    def log_p(self) -> int:
        return int(self.lut.shape[-1]).bit_length() - 1

    @property
    def out_image(self):
        """(outH, outW) of the valid correlation"""
        return self.image[0] - self.kernels.shape[2] + 1, self.image[1] - self.kernels.shape[3] + 1

    def luts(self) -> np.ndarray:
        """[outputs][2^log_p]: the shared table repeated, or the per-output tables"""
        return self.lut if self.lut.ndim == 2 else np.broadcast_to(self.lut, (self.outputs, self.lut.size))

    def weight_polys(self, N: int) -> np.ndarray:
        """[outputs][channels][N] int32: tap (dy, dx) at coefficient (kh-1-dy) W + (kw-1-dx)"""
        (h, wd), (kh, kw) = self.image, self.kernels.shape[2:]
        if h * wd > N:
            raise ValueError(f"an image of {h} x {wd} pixels does not fit {N} coefficients")
        polys = np.zeros(self.kernels.shape[:2] + (N,), dtype=np.int32)
        for dy in range(kh):
            for dx in range(kw):
                polys[:, :, (kh - 1 - dy) * wd + (kw - 1 - dx)] = self.kernels[:, :, dy, dx]
        return polys

    def output_indices(self) -> np.ndarray:
        """[outH * outW] in (y, x) order: output (y, x) sits at coefficient (y+kh-1) W + (x+kw-1)"""
        wd, (kh, kw), (oh, ow) = self.image[1], self.kernels.shape[2:], self.out_image
        y, x = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
        return ((y + kh - 1) * wd + (x + kw - 1)).reshape(-1).astype(np.uint32)

    def pack(self, images, N: int) -> np.ndarray:
        """images [..][H][W] -> message polynomials [..][N], pixel (y, x) at coefficient y W + x, zero above H W"""
        img = np.asarray(images)
        if tuple(img.shape[-2:]) != self.image:
            raise ValueError(f"images [..][{self.image[0]}][{self.image[1]}] expected")
        out = np.zeros(img.shape[:-2] + (N,), dtype=img.dtype)
        out[..., :self.image[0] * self.image[1]] = img.reshape(img.shape[:-2] + (-1,))
        return out

    def pre_activations(self, images) -> np.ndarray:
        """images [..][channels][H][W] integers -> the valid correlation + bias [..][outputs][outH][outW], unbounded integers"""
        img = np.asarray(images, dtype=np.int64)
        if tuple(img.shape[-3:]) != (self.channels,) + self.image:
            raise ValueError(f"images [..][{self.channels}][{self.image[0]}][{self.image[1]}] expected")
        (kh, kw), (oh, ow) = self.kernels.shape[2:], self.out_image
        k = self.kernels.astype(np.int64)
        out = np.zeros(img.shape[:-3] + (self.outputs, oh, ow), dtype=np.int64)
        for dy in range(kh):
            for dx in range(kw):
                # [.., 1, C, oh, ow] * [O, C, 1, 1] summed over C
                out += (img[..., None, :, dy:dy + oh, dx:dx + ow] * k[:, :, dy, dx][:, :, None, None]).sum(axis=-3)
        return out + self.bias[:, None, None]

    def pre_activation_range(self, lo, hi):
        """interval arithmetic: every pixel in [lo, hi] (scalars) -> (min, max) [outputs] of the pre-activations"""
        w = self.kernels.astype(np.int64).reshape(self.outputs, -1)
        pos, neg = np.maximum(w, 0).sum(axis=1), np.minimum(w, 0).sum(axis=1)
        lo, hi = int(lo), int(hi)
        return pos * lo + neg * hi + self.bias, pos * hi + neg * lo + self.bias

    def squared_norms(self) -> np.ndarray:
        """[outputs]: sum_c ||W[o][c]||_2^2, what an output multiplies the input noise's variance by"""
        return (self.kernels.astype(np.float64) ** 2).reshape(self.outputs, -1).sum(axis=1)

    def evaluate_clear(self, images) -> np.ndarray:
        """images [..][channels][H][W] integer messages -> the layer's messages [..][outputs][outH][outW] (run() returns
        them flattened in (o, y, x) order).  A pre-activation outside [0, 2^log_p) raises: check() tells beforehand."""
        pre = self.pre_activations(images)
        if int(pre.min()) < 0 or int(pre.max()) >= 1 << self.log_p:
            raise ValueError(f"pre-activation {int(pre.min() if pre.min() < 0 else pre.max())} outside [0, 2^{self.log_p})")
        return self.luts()[np.arange(self.outputs)[:, None, None], pre]

    def check(self, params, input_range=(0, 1)):
        """Raises ValueError unless the image fits the ring, the table matches params.log_p and, for pixels in
        input_range = (lo, hi), every pre-activation PROVABLY stays in [0, 2^log_p)"""
        if self.image[0] * self.image[1] > 1 << params.glwe_poly_degree:
            raise ValueError(f"an image of {self.image[0]} x {self.image[1]} pixels does not fit N = {1 << params.glwe_poly_degree}")
        if self.log_p != params.log_p:
            raise ValueError(f"the tables have 2^{self.log_p} entries, the parameter set has log_p = {params.log_p}")
        lo, hi = input_range
        if lo < 0 or hi >= 1 << params.log_p or lo > hi:
            raise ValueError(f"input_range must lie in [0, 2^{params.log_p})")
        pmin, pmax = self.pre_activation_range(lo, hi)
        bad = np.nonzero((pmin < 0) | (pmax >= 1 << params.log_p))[0]
        if bad.size:
            o = int(bad[0])
            raise ValueError(f"output {o}: pre-activations range over [{int(pmin[o])}, {int(pmax[o])}], outside [0, 2^{params.log_p})")

    def device_arrays(self, params):
        """(weight polynomials [O][C][N] int32, bias [O][N] uint32 ENCODED on the read coefficients, test vectors [O][N]
        or [N] un-encoded, output indices [outH outW])"""
        from . import construct_test_from_lut
        N = 1 << params.glwe_poly_degree
        idx = self.output_indices()
        bias = np.zeros((self.outputs, N), dtype=np.uint32)
        bias[:, idx] = ((self.bias << (32 - params.log_p - params.padding_bits)) & 0xFFFFFFFF).astype(np.uint32)[:, None]
        if self.lut.ndim == 1:
            tv = construct_test_from_lut(params, self.lut.astype(np.uint32))
        else:
            tv = np.stack([construct_test_from_lut(params, row.astype(np.uint32)) for row in self.lut])
        return self.weight_polys(N), bias, tv, idx

    def pre_activation_ciphertexts(self, ctx, glwe, weights=None):
        """glwe [queries][channels][k+1][N] -> the pre-activations as LWE ciphertexts [queries][O outH outW][k N + 1]
        before any key switch or bootstrap: glwe_conv, then sample_extract_indices.  `weights`: the PolyWeights of
        device_arrays()[0], prepared once by the caller; else they are prepared (and released) here."""
        polys, bias, _, idx = self.device_arrays(ctx.params)
        own = weights is None
        if own:
            weights = ctx.prepare_poly_weights(polys)
        try:
            is_torch = type(glwe).__module__.startswith("torch")
            if is_torch:
                import torch
                bias = torch.from_numpy(bias.view(np.int32)).to(glwe.device)
                idx = torch.from_numpy(idx.view(np.int32)).to(glwe.device)
            conv = ctx.glwe_conv(glwe, weights, bias)
            q = int(conv.shape[0])
            lwe = ctx.sample_extract_indices(conv.reshape((q * self.outputs,) + tuple(conv.shape[2:])), idx)
            if is_torch and own:
                torch.cuda.current_stream().synchronize()  # the weights go away with this call
            return lwe.reshape(q, self.outputs * int(idx.shape[0]), -1)
        finally:
            if own:
                weights.close()

    def run(self, ctx, glwe, weights=None):
        """glwe [queries][channels][k+1][N] (numpy: host forms; torch: device forms in the workspaces of
        ctx.reserve_glwe_conv and ctx.reserve) -> LWE ciphertexts [queries][O outH outW][io_dim + 1] in (o, y, x) order:
        glwe_conv, sample_extract_indices, a key switch in the reference's bootstrap order (which takes n + 1 words; the
        KS-first order takes the extracted k N + 1 words as they are), then one bootstrap per output pixel"""
        lwe = self.pre_activation_ciphertexts(ctx, glwe, weights)
        q, per_query = int(lwe.shape[0]), int(lwe.shape[1])
        flat = lwe.reshape(q * per_query, -1)
        if ctx.io_dim != ctx.params.big_n:
            flat = ctx.key_switch(flat)
        tv = self.device_arrays(ctx.params)[2]
        if tv.ndim == 2:  # bootstrap r = (query, output, pixel) takes output (r / pixels) % O's test vector
            tv = np.ascontiguousarray(np.broadcast_to(tv[None, :, None, :], (q, self.outputs, per_query // self.outputs, tv.shape[1]))
                                      ).reshape(q * per_query, -1)
        if type(flat).__module__.startswith("torch"):
            import torch
            tv = torch.from_numpy(tv.view(np.int32)).to(flat.device)
        return ctx.bootstrap(flat, tv).reshape(q, per_query, -1)


class Network:
    def __init__(self, layers):
        self.layers = list(layers)
        if not self.layers or any(not isinstance(layer, Dense) for layer in self.layers):
            raise ValueError("a non-empty list of Dense layers expected")
        for a, b in zip(self.layers, self.layers[1:]):
            if a.outputs != b.inputs:
                raise ValueError(f"a layer of {a.outputs} outputs feeds one of {b.inputs} inputs")
            if a.lut.shape[-1] != b.lut.shape[-1]:
                raise ValueError("all layers must use one message space (tables of one length)")

    @property
    def log_p(self) -> int:
        return int(self.layers[0].lut.shape[-1]).bit_length() - 1

    def evaluate_clear(self, x, all_layers: bool = False):
        """x [..][inputs] integer messages -> the last layer's messages, or (all_layers) every layer's in a list.  A
        pre-activation outside [0, 2^log_p) raises: check() tells beforehand whether one can occur."""
        outs = []
        x = np.asarray(x, dtype=np.int64)
        for n, layer in enumerate(self.layers):
            pre = layer.pre_activations(x)
            if int(pre.min()) < 0 or int(pre.max()) >= 1 << self.log_p:
                raise ValueError(f"layer {n}: pre-activation {int(pre.min() if pre.min() < 0 else pre.max())} outside [0, 2^{self.log_p})")
            x = layer.luts()[np.arange(layer.outputs), pre]  # out[.., o] = lut_o[pre[.., o]]
            outs.append(x)
        return outs if all_layers else x

    def check(self, params, input_range=(0, 1)):
        """Raises ValueError unless, for inputs in input_range = (lo, hi) (scalars or one pair per input), every
        pre-activation of every row of every layer PROVABLY stays in [0, 2^log_p): interval arithmetic over the rows,
        a layer's outputs ranging over the entries of its table(s).  Also: the tables match params.log_p, and no neuron
        can hand 2^31 to an odd weight of the next layer (the module's text)."""
        if self.log_p != params.log_p:
            raise ValueError(f"the tables have 2^{self.log_p} entries, the parameter set has log_p = {params.log_p}")
        lo, hi = input_range
        if np.any(np.asarray(lo) < 0) or np.any(np.asarray(hi) >= 1 << params.log_p) or np.any(np.asarray(lo) > np.asarray(hi)):
            raise ValueError(f"input_range must lie in [0, 2^{params.log_p})")
        for n, layer in enumerate(self.layers):
            pmin, pmax = layer.pre_activation_range(lo, hi)
            bad = np.nonzero((pmin < 0) | (pmax >= 1 << params.log_p))[0]
            if bad.size:
                o = int(bad[0])
                raise ValueError(f"layer {n}, row {o}: pre-activations range over [{int(pmin[o])}, {int(pmax[o])}], outside "
                                 f"[0, 2^{params.log_p})")
            if n + 1 < len(self.layers):  # the padding bit between layers (see the module's text)
                odd = (self.layers[n + 1].weights.astype(np.int64) & 1).any(axis=0)
                bad = np.nonzero((layer.luts()[:, 0] != 0) & (pmin <= 0) & odd)[0]
                if bad.size:
                    raise ValueError(f"layer {n}, row {int(bad[0])}: lut[0] != 0 on a pre-activation that can be 0, under an odd "
                                     f"weight of layer {n + 1}: its output may carry 2^31 into the next padding bit")
            lo, hi = layer.luts().min(axis=1), layer.luts().max(axis=1)

    def noise_bound(self, params, sigma_in: float, ks_first: bool = False):
        """Per layer, the predicted standard deviations in units of the 32-bit torus (sigma_in likewise, e.g.
        params.lwe_std_dev * 2^32), the largest over the layer's rows:
          sigma_pre  before the rotation: sigma^2 = ||W_o||_2^2 sigma_in^2 (+ the key switch's term in the KS-first order)
          sigma_out  of the layer's outputs, the next layer's sigma_in: the rotation's term (+ the key switch's in the
                     reference's order) -- a bootstrap's output noise does not depend on its input's
        with the terms of DESIGN.md section 8: s_br^2 = n [(k+1) l N (B^2/12 + 1/6)(sigma_glwe 2^32)^2 + (1 + kN/2)
        2^(2 ig)/12], s_ks^2 = kN l_ks (B_ks^2/12 + 1/6)(sigma_lwe 2^32)^2 + (kN/2) 2^(2 ig_ks)/12.
        -> [{"sigma_pre": .., "sigma_out": ..}, ..]"""
        k, N, n = params.glwe_dimension, 1 << params.glwe_poly_degree, params.lwe_dimension
        pbs, ks = params.pbs_decomposer, params.ks_decomposer

        def digit_sq(d):
            return float(1 << d.log_base) ** 2 / 12.0 + 1.0 / 6.0

        ig_pbs, ig_ks = 32 - pbs.log_base * pbs.levels, 32 - ks.log_base * ks.levels
        s_br = n * ((k + 1) * pbs.levels * N * digit_sq(pbs) * (params.glwe_std_dev * 2.0 ** 32) ** 2
                    + (1 + k * N / 2.0) * 2.0 ** (2 * ig_pbs) / 12.0)
        s_ks = k * N * ks.levels * digit_sq(ks) * (params.lwe_std_dev * 2.0 ** 32) ** 2 + (k * N / 2.0) * 2.0 ** (2 * ig_ks) / 12.0
        out = []
        var_in = float(sigma_in) ** 2
        for layer in self.layers:
            var_pre = float(layer.squared_norms().max()) * var_in + (s_ks if ks_first else 0.0)
            var_out = s_br + (0.0 if ks_first else s_ks)
            out.append({"sigma_pre": math.sqrt(var_pre), "sigma_out": math.sqrt(var_out)})
            var_in = var_out
        return out

    def device_arrays(self, params):
        """per layer (weights [O][I] int32, bias [O] uint32 ENCODED, test vectors [O][N] or [N] un-encoded): what
        Context.dense_bootstrap takes"""
        from . import construct_test_from_lut
        shift = 32 - params.log_p - params.padding_bits
        arrays = []
        for layer in self.layers:
            bias = ((layer.bias << shift) & 0xFFFFFFFF).astype(np.uint32)
            if layer.lut.ndim == 1:
                tv = construct_test_from_lut(params, layer.lut.astype(np.uint32))
            else:
                tv = np.stack([construct_test_from_lut(params, row.astype(np.uint32)) for row in layer.lut])
            arrays.append((layer.weights, bias, tv))
        return arrays

    def run(self, ctx, cts, all_layers: bool = False, arrays=None):
        """cts [queries][inputs][io_dim + 1] (numpy: host forms; torch: device forms in the workspace of
        ctx.reserve_dense, `arrays` may name device copies of device_arrays(), else they are uploaded per call) ->
        the last layer's ciphertexts [queries][outputs][io_dim + 1], or (all_layers) every layer's in a list: ONE
        dense_bootstrap per layer"""
        arrays = arrays if arrays is not None else self.device_arrays(ctx.params)
        outs = []
        for weights, bias, tv in arrays:
            cts = ctx.dense_bootstrap(cts, weights, bias, tv)
            outs.append(cts)
        return outs if all_layers else cts
