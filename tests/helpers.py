"""Shared test helpers: golden loading, seeded inputs (same recipe as tests/golden/make_golden.py)."""
import json
import os
import types

import numpy as np
import torch

import airnet_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

VARIANTS = {
    'all3': dict(degradation_embedding_method=['all_3_bands'], L=3, encoder_msa_type='freq'),
    'allDC': dict(degradation_embedding_method=['all_DC'], L=3, encoder_msa_type='freq'),
    'all2_L2': dict(degradation_embedding_method=['all_2_bands'], L=2, encoder_msa_type='freq'),
    'all3_origin': dict(degradation_embedding_method=['all_3_bands'], L=3, encoder_msa_type='origin'),
}


def load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False) as z:
        return {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind != 'U' else z[k]) for k in z.files}


def schema(variant):
    with open(os.path.join(GOLDEN, 'schema.json')) as f:
        return [tuple(e) for e in json.load(f)[variant]]


def rnd(name, shape, scale=1.0):
    return O.seeded_tensor('input.' + name, shape) / 0.02 * scale


def synth_batch(B, size, tag):
    clean = torch.sigmoid(rnd(tag + 'clean', (B, 3, size, size), 1.5))
    q = (clean + rnd(tag + 'nq', clean.shape, 25 / 255.)).clamp(0, 1)
    k = (clean + rnd(tag + 'nk', clean.shape, 25 / 255.)).clamp(0, 1)
    return clean, q, k


def make_opt(variant, batch_size=2, **kw):
    d = dict(L=3, encoder_dim=256, encoder_embed_dim=28, embed_dim=56, batch_size=batch_size, patch_size=128,
             contrast_loss_weight=0.6, encoder_type='Uformer', decoder_type='Uformer', debug_mode=False,
             frequency_decompose_type='none', learnable_modulator=False, compute_dtype='fp32')
    d.update(VARIANTS[variant])
    d.update(kw)
    return types.SimpleNamespace(**d)


def close(a, b, tol, what=''):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, f'{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}'
    assert torch.isfinite(a).all(), f'{what}: non-finite values'
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item() / scale
    assert err < tol, f'{what}: rel-to-max err {err:.3e} >= {tol:.1e} (scale {scale:.3e})'
    return err


def kdiff_state(variant='all3'):
    """Seeded state whose key encoder keeps its OWN name-seeded weights (golden model_all3_kdiff: the contrastive loss is O(1))."""
    sch = schema(variant)
    st = O.fill_state_seeded(sch)
    for name, shape, _ in sch:
        if name.startswith('E.E.encoder_k.') and O.is_parameter_key(name):
            st[name] = O.seeded_tensor(name, tuple(shape))
    return st


# golden model_all3_kdiff: gradient norms of the three 448 -> 65 536 head weights evaluated in FLOAT64 by the oracle (same graph, same
# weights).  dW = sum_t dY[t]^T xn[t] with sum_t dY[t] = 0 (BatchNorm backward) and xn[t] almost equal for all tokens (name-seeded
# weights): the sum is what survives a cancellation, and the reference's own f32 evaluation (torch CPU) is 0.24 .. 0.41 % away from
# the f64 value.  tests/test_oracle_model.py re-derives these constants; the HIP f32 path (exact-f32 MFMA products) must match THEM.
KDIFF_HEAD_WEIGHT_NORMS_F64 = {
    'E.E.encoder_q.mlp_head.0.1.weight': 0.028330916389931654,
    'E.E.encoder_q.mlp_head.1.1.weight': 0.03231436757293798,
    'E.E.encoder_q.mlp_head.2.1.weight': 0.015436637595669512,
}


# ------------------------------------------------------------------------------------------------ GEMM error bound
# fw_gemm computes  C = epilogue(alpha * sum_k X(m,k) W(n,k))  with operands already rounded to their storage type and an f32
# accumulator.  For ANY order of summation (MFMA chains, K split over workgroups, atomicAdd of split-K slices) the computed f32 sum s
# satisfies  |s - sum| <= gamma_K * sum_k |x_k w_k|,  gamma_K = K u / (1 - K u),  u = 2^-24  (Higham, Accuracy and Stability of
# Numerical Algorithms, section 3.1: one rounding per product -- none for bf16 operands, whose products are exact in f32 -- and at most
# K - 1 per term for the additions).  The epilogue adds at most four more f32 operations on the sum (times alpha, plus bias, times the
# row scale, plus the residual or the value the output already holds), each one rounding relative to a partial result that the same
# magnitude sum bounds: K + 4.  The second-order part of (1 + u)^(K + 4) - 1 is below (K u)^2 / 2 < 0.1 u for K <= 2048; MFMA products
# of f32 operands add their own rounding (already counted in gamma_K) and the f32 -> f64 comparison itself none.  c = 8 is twice what
# the count needs; it is NOT fitted to any run.
U32 = 2.0 ** -24                  # unit roundoff of f32
UBF = 2.0 ** -8                   # unit roundoff of bf16 (8 significant bits, round to nearest even)
GEMM_EPI_ROUNDINGS = 8
# approximation errors stated in csrc/fw_common.h:81-100
ERF_ABS_ERR = 1.5e-7              # Abramowitz-Stegun 7.1.26
# erf_fast evaluated in f32: v_rcp (1 ulp), v_exp (1 ulp), five Horner steps, the products around them: <= 16 roundings of
# quantities <= 1.5 in magnitude
ERF_EVAL_ERR = 16 * U32
GELU_POLY_ABS_ERR = 5e-5          # bf16 polynomial GELU on [-4, 4]
GELU_POLY_REL_ERR = 4e-5          # ... and 4e-5 |x| beyond
GELU_GRAD_POLY_ERR = 3e-4         # bf16 polynomial GELU'
POLY_EVAL_ROUNDINGS = 16          # degree-7 Horner in f32: 8 fma, the clamp, x^2, two more products
GELU_LIPSCHITZ = 1.13             # sup |GELU'| = 1.1290 (at x = sqrt(2))


def gelu64(v):
    return 0.5 * v * (1 + torch.erf(v / 2 ** 0.5))


def gelu_grad64(v):
    return 0.5 * (1 + torch.erf(v / 2 ** 0.5)) + v * torch.exp(-0.5 * v * v) / (2 * torch.pi) ** 0.5


def gelu_value_err(v, dtype):
    """|kernel GELU(v) - GELU(v)| for an exact f32 argument v (f64 tensor of its magnitudes is enough), before any output rounding"""
    a = v.abs()
    if dtype == torch.bfloat16:
        return torch.maximum(torch.full_like(a, GELU_POLY_ABS_ERR), GELU_POLY_REL_ERR * a) + POLY_EVAL_ROUNDINGS * U32 * a
    return 0.5 * a * (ERF_ABS_ERR + ERF_EVAL_ERR) + 3 * U32 * a          # 0.5 * v * (1 + erf): three more roundings of |.| <= |v|


def gelu_grad_value_err(dtype):
    """|kernel GELU'(x) - GELU'(x)|: polynomial (bf16) or cdf + x * pdf in f32 (|x pdf| (2 + x^2) <= 0.83: exp argument and value
    roundings stay below 4 u)"""
    return GELU_GRAD_POLY_ERR if dtype == torch.bfloat16 else 0.5 * (ERF_ABS_ERR + ERF_EVAL_ERR) + 4 * U32


def gelu_operand_err(w, dtype):
    """|operand the kernel multiplies - GELU(w)| when GELU is applied while the operand is staged (x_op / w_op = 1): the value error
    and, in bf16, the re-rounding of the result to the storage type (one bf16 ulp of it)"""
    e = gelu_value_err(w, dtype)
    if dtype == torch.bfloat16:
        e = e + 2 * UBF * (gelu64(w).abs() + e)
    return e


class GemmRef:
    """f64 reference of one product: acc = alpha * X W^T and the magnitude sum mag = |alpha| |X| |W|^T the bound is relative to.
    x: [M, K], w: [N, K] float64 tensors holding the storage-rounded operand values (host or device)."""

    def __init__(self, x, w, alpha=1.0, operand_err=None):
        self.x, self.w, self.alpha, self.K = x, w, float(alpha), x.shape[1]
        self.acc = self.alpha * (x @ w.t())
        self.mag = abs(self.alpha) * (x.abs() @ w.abs().t())
        self.operand_err = operand_err           # [M, N] bound of |alpha| sum_k |x_k| |w~_k - w_k| (operand transformed by the kernel)

    def without_term(self, k0):
        """the same product one k term short (what a dropped K tail or a skipped ring stage computes)"""
        r = object.__new__(GemmRef)
        r.__dict__.update(self.__dict__)
        r.acc = self.acc - self.alpha * torch.outer(self.x[:, k0], self.w[:, k0])
        return r

    def probe_ks(self, kstep):
        """the last k, and one in the middle of the last K step of `kstep` elements"""
        first = (self.K - 1) // kstep * kstep
        return [self.K - 1, first + (self.K - first) // 2]


def gemm_expect(ref, dtype, *, bias=None, act=0, aux=None, rowscale=None, residual=None, prefill=None, out_bf16=False, twin=False):
    """-> {'out': (value, tol, gain)[, 'twin': (value, tol, gain)]}: what fw_gemm's epilogue makes of ref.acc in exact arithmetic, the
    element-wise bound of the kernel's deviation from it, and |d value / d acc| (how much of a change of the sum the output shows).
    bias [N], rowscale [M] (already expanded per row), residual / prefill / aux [M, N]: float64."""
    g = (ref.K + GEMM_EPI_ROUNDINGS) * U32
    v, mag = ref.acc, ref.mag
    if bias is not None:
        v, mag = v + bias, mag + bias.abs()
    tol = g * mag
    if ref.operand_err is not None:
        tol = tol + ref.operand_err
    gain = torch.ones_like(v)
    if act == 2:
        gp, eg = gelu_grad64(aux), gelu_grad_value_err(dtype)
        tol = tol * (gp.abs() + eg) + v.abs() * eg
        v, gain = v * gp, gp.abs()
    elif act == 3:
        tol = GELU_LIPSCHITZ * tol + gelu_value_err(v.abs() + tol, dtype)
        v, gain = gelu64(v), gelu_grad64(v).abs()
    if rowscale is not None:
        v, tol, gain = v * rowscale[:, None], tol * rowscale[:, None].abs(), gain * rowscale[:, None].abs()
    for add in (residual, prefill):
        if add is not None:
            v, tol = v + add, tol + g * add.abs()
    res = {}
    if twin:                                                   # second output GELU(v), in the operand type
        t_tol = GELU_LIPSCHITZ * tol + gelu_value_err(v.abs() + tol, dtype)
        t_val = gelu64(v)
        if dtype == torch.bfloat16:
            t_tol = t_tol + UBF * (t_val.abs() + t_tol)
        res['twin'] = (t_val, t_tol, gain * gelu_grad64(v).abs())
    if out_bf16:
        tol = tol + UBF * (v.abs() + tol)
    res['out'] = (v, tol, gain)
    return res


def bound_violations(y, value, tol):
    """element-wise |y - value| > tol over the WHOLE output (non-finite y counts as a violation)"""
    y = y.detach().to(value.device, torch.float64)
    assert y.shape == value.shape, f'shape {tuple(y.shape)} vs {tuple(value.shape)}'
    return ~((y - value).abs() <= tol)


def assert_within_bound(y, value, tol, what=''):
    bad = bound_violations(y, value, tol)
    n = int(bad.sum())
    if n:
        err = (y.detach().to(value.device, torch.float64) - value).abs()
        ratio = torch.where(bad, torch.nan_to_num(err / tol, nan=float('inf'), posinf=float('inf')), torch.zeros_like(err))
        i = int(ratio.argmax())
        m, c = divmod(i, value.shape[1])
        raise AssertionError(f'{what}: {n} of {bad.numel()} elements outside the derived bound; worst at [{m}, {c}]: '
                             f'got {float(y[m, c]):.9g}, reference {float(value[m, c]):.9g}, bound {float(tol[m, c]):.3e}')


GEMM_MIN_REJECTED = 0.99
# An epilogue that is not linear in the sum shows a change of the sum scaled by its derivative: v * GELU'(aux) by GELU'(aux), GELU(v)
# by GELU'(v).  Both derivatives are >= 0.5 exactly where their argument is >= 0, which a symmetric aux or sum is at half of the
# elements; the share asked of the selection is a little under that half.
GEMM_MIN_GAIN = 0.5
GEMM_MIN_SELECTED = 0.4


def rejected_share(y, value, tol, gain=None):
    """-> (rejected, selected): the share of the selected elements at which the bound REJECTS y against this reference, and the share
    of all elements that is selected: every one, or with `gain` those whose epilogue passes at least GEMM_MIN_GAIN of a change of the
    sum on.  An empty selection rejects nothing."""
    bad = bound_violations(y, value, tol)
    if gain is None:
        return float(bad.double().mean()), 1.0
    sel = gain >= GEMM_MIN_GAIN
    n = int(sel.sum())
    return (float(bad[sel].double().mean()) if n else 0.0), n / sel.numel()


def signed_magnitudes(*shape, seed=0, lo=0.75, hi=1.25, sign=0):
    """operands for the GEMM bound tests: random sign (or the one given: +1, -1), magnitude uniform in [lo, hi).  Every k term
    |x w| >= lo^2 = 0.5625 then stands clear of the bound (gamma * K * E|x w| = 0.21 at K = 1856, plus 2^-8 |ref| ~ 0.17 for a bf16
    output), which plain N(0, 1) operands do not give: the product of two normals is below 0.13 -- the bound at that K -- for a
    quarter of all (m, n).  In bf16 these products are multiples of 2^-16 and the sums stay below 2^6, so an f32 accumulator holds
    almost every partial sum exactly: bf16 runs show that a kernel is not wrong by a term, not that the (K + 8) 2^-24 part of the
    bound is tight; only the f32 cases load that part."""
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape))
    mag = lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float32)
    rnd_sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return mag * (rnd_sign if sign == 0 else sign)


def check_gemm(ref, dtype, outputs, what, min_rejected=GEMM_MIN_REJECTED, **epi):
    """outputs: {'out': tensor[, 'twin': tensor]} as a kernel wrote them; epi: the epilogue, as gemm_expect takes it.  Every element
    must lie within the bound of the reference, and the bound must REJECT the same outputs against the reference one k term short
    (the last k; one in the middle of the last 128-byte K step) at `min_rejected` of the elements (see rejected_share)."""
    exp = gemm_expect(ref, dtype, **epi)
    linear = epi.get('act', 0) == 0
    for key, y in outputs.items():
        value, tol, _ = exp[key]
        assert_within_bound(y, value, tol, f'{what} [{key}]')
    for k0 in ref.probe_ks(128 // (2 if dtype == torch.bfloat16 else 4)):
        short = gemm_expect(ref.without_term(k0), dtype, **epi)
        for key, y in outputs.items():
            value, tol, _ = short[key]
            share, selected = rejected_share(y, value, tol, None if linear and key == 'out' else exp[key][2])
            assert selected >= GEMM_MIN_SELECTED, (f'{what} [{key}]: only {selected:.4f} of the elements pass {GEMM_MIN_GAIN} of a change of '
                                                   f'the sum on (asked: {GEMM_MIN_SELECTED}); the missing-term check would cover too few')
            assert share >= min_rejected, (f'{what} [{key}]: the bound tells the output from a reference without the k = {k0} term at '
                                           f'{share:.4f} of the {selected:.4f} of the elements it is asked at (asked: {min_rejected})')
