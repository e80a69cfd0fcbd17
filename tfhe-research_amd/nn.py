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
