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


# ------------------------------------------------------------------------------------------------ per-step kernels (csrc/fw_elem.hip)
# Guarded buffers: every output is allocated GUARD elements larger on both sides and pre-filled with SENTINEL, the kernel gets the
# inner view, and the whole buffer is compared bit for bit with what it must hold afterwards.  GUARD = 8 keeps an f32 or bf16 view
# that starts right behind it 16-byte aligned; an extra offset k then makes the base pointer as unaligned as the case asks.
SENTINEL = 7.0
GUARD = 8
F32_TINY = 2.0 ** -126            # smallest normal f32: a result below it may be flushed or lose bits, |error| <= F32_TINY per operation


def guarded(n, dtype, device, k=0):
    """-> (buf, view): buf = SENTINEL everywhere, GUARD + k elements before and GUARD after view = buf[GUARD + k : GUARD + k + n]"""
    buf = torch.full((GUARD + k + n + GUARD,), SENTINEL, dtype=dtype, device=device)
    return buf, buf[GUARD + k:GUARD + k + n]


def guarded_like(values, device, k=0):
    """guarded buffer whose inner view holds `values` (1-D host tensor)"""
    buf, view = guarded(values.numel(), values.dtype, device, k)
    view.copy_(values)
    return buf, view


def bits(t):
    """integer view of a tensor's storage bits (host copy)"""
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bits(got, want, what=''):
    """bit-for-bit equality (so -0.0 != 0.0, and a NaN is equal to the same NaN)"""
    assert got.shape == want.shape and got.dtype == want.dtype, f'{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}'
    a, b = bits(got), bits(want)
    bad = a != b
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits; first at flat index {i}: '
                             f'got {got.detach().cpu().reshape(-1)[i].item()!r}, want {want.detach().cpu().reshape(-1)[i].item()!r}')


def assert_guarded(buf, inner, k=0, what=''):
    """buf (from guarded(.., k)) holds `inner` in its view and SENTINEL everywhere else, bit for bit"""
    want = torch.full(buf.shape, SENTINEL, dtype=buf.dtype)
    want[GUARD + k:GUARD + k + inner.numel()] = inner.detach().cpu().reshape(-1).to(buf.dtype)
    assert_bits(buf, want, what)


def assert_bound_1d(y, value, tol, what=''):
    """every element of y within tol of value (f64 host tensors of any shape; non-finite y fails)"""
    y = y.detach().cpu().double().reshape(-1)
    value, tol = value.reshape(-1), tol.reshape(-1)
    bad = ~((y - value).abs() <= tol)
    if bool(bad.any()):
        ratio = torch.where(bad, torch.nan_to_num((y - value).abs() / tol, nan=float('inf'), posinf=float('inf')), torch.zeros_like(tol))
        i = int(ratio.argmax())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements outside the derived bound; worst at [{i}]: '
                             f'got {float(y[i]):.9g}, reference {float(value[i]):.9g}, bound {float(tol[i]):.3e}')


def outside_share(y, value, tol):
    """share of the elements of y that the bound rejects against this reference"""
    y = torch.as_tensor(y).detach().cpu().double().reshape(-1)
    return float((~((y - value.reshape(-1)).abs() <= tol.reshape(-1))).double().mean())


# ---- Adam.  adam_kernel evaluates, in f32 and per element,
#     mi = m * b1 + g * (1 - b1);  vi = v * b2 + g * g * (1 - b2);  denom = sqrtf(vi) / sqrtf(1 - hyper[2]) + eps;
#     p' = p - (hyper[0] / (1 - hyper[1])) * (mi / denom)
# The reference evaluates the same expression in f64 from the f32 inputs (b1, b2, eps as the f32 values the ABI receives).  The bound
# counts the kernel's roundings, u = 2^-24 each; contracting a product and a sum into one fma only removes roundings.
ADAM_M_ROUNDINGS = 4              # 1 - b1, the two products, their sum
ADAM_V_ROUNDINGS = 5              # 1 - b2, g * g, times (1 - b2), v * b2, their sum (all terms >= 0: relative to vi itself)
SQRTF_ERR = 2 * U32               # sqrtf: 1 ulp (HIP's documented bound; the default build rounds it correctly, 0.5 ulp)
DIV_ERR = 2 * U32                 # f32 division: 1 ulp (same remark); there are two: hyper[0] / bc1 and mi / denom
ADAM_BC_ROUNDINGS = 1             # 1 - hyper[1] and 1 - hyper[2]: one rounding each (halved by the square root for the latter)
ADAM_EPS_SUM_ROUNDINGS = 1        # ... + eps
ADAM_SCALE_ROUNDINGS = 1          # (lr / bc1) * (mi / denom)
ADAM_P_ROUNDINGS = 1              # the final rounding of p - update, relative to the result
SECOND_ORDER = 1 + 2.0 ** -10     # the products of two error terms the first-order count drops are below 2^-20 of it


def f32c(x):
    """the f32 value a C float argument receives, as a Python float"""
    return float(np.float32(x))


def adam_reference(p, g, m, v, hyper, b1, b2, eps):
    """p, g, m, v: f64 tensors holding f32 values; hyper: the four f32 values {lr, beta1^t, beta2^t, t} the kernel reads.
    -> dict m, v, p (the f64 results) and tol_m, tol_v, tol_p (element-wise bounds of the kernel's deviation from them)."""
    b1, b2, eps = f32c(b1), f32c(b2), f32c(eps)
    lr, h1, h2 = (float(hyper[i]) for i in range(3))
    am, bm = m * b1, g * (1 - b1)
    m1 = am + bm
    tol_m = ADAM_M_ROUNDINGS * U32 * (am.abs() + bm.abs()) + 3 * F32_TINY
    v1 = v * b2 + g * g * (1 - b2)
    tol_v = ADAM_V_ROUNDINGS * U32 * v1 + 4 * F32_TINY
    s = v1.sqrt()
    s_hi, s_lo = (v1 + tol_v).sqrt(), (v1 - tol_v).clamp(min=0).sqrt()
    ds = torch.maximum(s_hi - s, s - s_lo) + SQRTF_ERR * s_hi
    bc2s = (1 - h2) ** 0.5
    e_bc2s = 0.5 * ADAM_BC_ROUNDINGS * U32 + SQRTF_ERR
    q = s / bc2s
    dq = ds / bc2s + (s + ds) / bc2s * (e_bc2s + DIV_ERR)
    denom = q + eps
    dden = dq + ADAM_EPS_SUM_ROUNDINGS * U32 * (denom + dq)
    r = m1 / denom
    dr = tol_m / (denom - dden) + m1.abs() * dden / (denom * (denom - dden)) + DIV_ERR * (m1.abs() + tol_m) / (denom - dden) + F32_TINY
    c = lr / (1 - h1)
    e_c = ADAM_BC_ROUNDINGS * U32 + DIV_ERR
    upd = c * r
    dupd = abs(c) * (1 + e_c) * dr + upd.abs() * (e_c + ADAM_SCALE_ROUNDINGS * U32) + F32_TINY
    p1 = p - upd
    tol_p = (dupd + ADAM_P_ROUNDINGS * U32 * (p1.abs() + dupd)) * SECOND_ORDER
    return dict(m=m1, v=v1, p=p1, tol_m=tol_m * SECOND_ORDER, tol_v=tol_v * SECOND_ORDER, tol_p=tol_p)


def adam_f32(p, g, m, v, hyper, b1, b2, eps, mutation=None):
    """numpy f32 restatement of adam_kernel's expression (one rounding per operation), or of one of the wrong kernels the bound must
    reject: 'eps_in_sqrt', 'bc2_no_sqrt', 'b2_for_m', 'lr_no_bc1'.  Inputs: f32 numpy arrays.  -> (p', m', v') f32."""
    f = np.float32
    b1, b2, eps, one = f(b1), f(b2), f(eps), f(1)
    lr, bc1, bc2 = f(hyper[0]), one - f(hyper[1]), one - f(hyper[2])
    bc2_sqrt = bc2 if mutation == 'bc2_no_sqrt' else np.sqrt(bc2)
    bm = b2 if mutation == 'b2_for_m' else b1
    mi = m * bm + g * (one - bm)
    vi = v * b2 + g * g * (one - b2)
    denom = np.sqrt(vi + eps) / bc2_sqrt if mutation == 'eps_in_sqrt' else np.sqrt(vi) / bc2_sqrt + eps
    scale = lr if mutation == 'lr_no_bc1' else lr / bc1
    pi = p - scale * (mi / denom)
    assert pi.dtype == np.float32 and mi.dtype == np.float32 and vi.dtype == np.float32
    return pi, mi, vi


ADAM_SPECIAL = 24                 # elements at the front of adam_case that carry the edge values


def adam_case(n, seed, scale=1e-6):
    """Seeded f32 inputs (p, g, m, v) of n elements.  |g| in [1, 2) scale, |m| in [0.25, 0.75) scale, v in [0.5, 1.5) scale^2, random
    signs, |p| in [0.25, 1): at scale 1e-6 sqrt(v) is of the order of eps = 1e-8 / its bias correction, so eps inside the root, a
    missing root of bc2 or a missing 1 / bc1 all move the update by a multiple of itself, and |m - g| >= scale / 4 keeps
    (b2 - b1)(m - g) -- what b2 in place of b1 changes -- away from zero: every one of those wrong kernels moves p by far more than
    u |p| (tests/test_step_bounds_cpu.py checks it).  The first min(n, ADAM_SPECIAL) elements cycle through the edges instead:
    g == 0, |g| = 1e-20 (g * g underflows), and m = v = 0 with each of them and with an ordinary g."""
    gen = torch.Generator().manual_seed(1000 * seed + n % 997)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64)
    sg = lambda: torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    p, g, m, v = u(0.25, 1) * sg(), u(1, 2) * scale * sg(), u(0.25, 0.75) * scale * sg(), u(0.5, 1.5) * scale * scale
    for i in range(min(n, ADAM_SPECIAL)):
        kind = i % 6
        if kind in (0, 3):
            g[i] = 0.0
        elif kind in (1, 4):
            g[i] = 1e-20 * (1 if i % 4 < 2 else -1)
        if kind >= 3:
            m[i] = 0.0; v[i] = 0.0
    return tuple(t.float().numpy() for t in (p, g, m, v))


# ---- EMA.  ema_kernel: x = pk * mom + pq * (1 - mom) in f32.  1 - mom is exact for mom in [0.5, 1] (Sterbenz); the reference takes
# its f32 value, so three roundings are left: the two products and the sum.
EMA_ROUNDINGS = 3


def ema_reference(pk, pq, mom):
    """pk, pq: f64 tensors of f32 values -> (x, tol)"""
    momf = np.float32(mom)
    a, b = pk * float(momf), pq * float(np.float32(1) - momf)
    x = a + b
    per_rounding = (a.abs(), b.abs(), x.abs())                    # each rounding is relative to the value it produces
    assert len(per_rounding) == EMA_ROUNDINGS
    return x, (U32 * sum(per_rounding) + EMA_ROUNDINGS * F32_TINY) * SECOND_ORDER


# ---- L1 loss.  l1_loss_kernel: a grid of min(ceil(n / 256), 1024) blocks of 256 threads; a thread adds |a - b| over its grid-stride
# elements, the 64 lanes of a wave are folded by 6 shuffle steps, the wave sum is divided by n and added to *loss with one atomic.
def l1_chain_length(n):
    """longest chain of f32 additions (and the other roundings on the way) between one |a - b| and the loss"""
    threads = min((n + 255) // 256, 1024) * 256
    per_thread = (n + threads - 1) // threads               # additions into the thread's partial sum
    wave_fold = 6
    atomics = threads // 64                                 # one atomicAdd per wave, in any order
    subtraction, division = 1, 1
    return subtraction + per_thread + wave_fold + division + atomics


def l1_loss_bound(a, b):
    """a, b: f64 host tensors of f32 values -> (loss, tol)"""
    n = a.numel()
    mag = float((a - b).abs().sum()) / n
    return mag, l1_chain_length(n) * U32 * mag * SECOND_ORDER
