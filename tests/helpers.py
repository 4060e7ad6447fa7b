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


# ------------------------------------------------------------------------------------------------ window attention (csrc/fw_attn.hip)
# Element-wise bounds of fw_attn_fwd / fw_attn_bwd.  The reference evaluates the operation in f64 from the storage-rounded operands
# and keeps every intermediate the kernels form (scores s, P, B1(P), P', dP', dS, lse); each bound below counts the roundings between
# that intermediate and the f64 value, read off the kernels (attn_*, attn2_*, attn2x_* share the arithmetic; they differ in the walk).
# u = U32 throughout; ut = the rounding of a value stored in the operand type before the next MFMA product or as an output.
# ut = UBF: v_cvt_pk_bf16_f32 rounds to nearest even (fw_common.h f2bf / pack_bf2), half an ulp of 8 significant bits
# scores: sum_d k q in an f32 MFMA chain (D terms; bf16 products are exact in f32, f32 ones round once), then  acc * scale,
# bias + (-100), and the sum of the two: D + 3 roundings of partial results that scale * sum |q||k| + |bias| + |mask| bounds
ATTN_SCORE_ROUNDINGS = 3
# exp argument x = s - max (forward) or s - lse (backward): the subtraction, the product with log2(e) inside __expf, and the f32
# value of log2(e) itself -- three roundings relative to |x|, i.e. a relative error 3 u |x| of exp(x)
ATTN_EXP_ARG_ROUNDINGS = 3
ATTN_EXP_VALUE_ERR = 2 * U32      # v_exp_f32: 1 ulp
ATTN_SUM_EXTRA = 2                # softmax sum: NK / 4 sequential additions per lane (positive terms), then 2 shuffle steps
ATTN_NORM_ERR = DIV_ERR + U32     # inv = 1.0f / sum (1 ulp) and p * inv
# lse = max + __logf(sum): v_log_f32 (1 ulp of log2 sum, and not better than 1 ulp of 1 when sum is just above 1), the product with
# ln 2 and ln 2's own f32 value: 4 u (1 + log sum); then the final sum, one rounding of |lse|
ATTN_LOG_ERR = 4 * U32
ATTN_COMBINE_ROUNDINGS = 3        # P' = p * a + b + f * c: each term passes at most three roundings (fewer when contracted to fma)
ATTN_ACC_EXTRA = 2                # a 64- or 128-term f32 MFMA chain: K roundings, + the scale product behind dq / dk, + slack of one
ATTN_DS_ROUNDINGS = 2             # dS = p * (dp - D_i): the difference (relative to |dp| + |D_i|) and the product
ATTN_LANE_TERMS = 16              # score elements a lane owns per key tile: its sequential partial sums are this long
ATTN_WAVE_FOLD = 6                # wave_sum: 6 shuffle steps
ATTN_BIN_FOLD = 64                # LDS atomics into one of the 225 relative positions: at most 64 (i, j) pairs share one (i == j)
# The ONE measured constant: the error of the partial-DFT band filter B1 (band_filter2: four MFMA stages; in bf16 the panels, the
# input and the stage outputs T, Y, Z are rounded to bf16).  Its worst-case chain is several times |B1(x)| itself (sum |x| * 2 / 4096
# * 45 * 23 * 8 per element), useless as a bound, and even the largest error of a map, carried element by element through the next
# 64-term product, swamps a filter term that is 10 % short.  What the outputs see is that error CONTRACTED with another operand:
# sum_j e_ij w_j.  The e_ij are rounding errors (round to nearest even: zero mean -- the measured mean is below 3 % of the rms --
# and not aligned with w), so the sum has the standard deviation sigma ||w||_2, sigma = the rms of e; the bound allows
# ATTN_FILTER_SIGMAS of them.  sigma is measured on the CPU, never on a GPU: fwair.lfs.emulate_filter with the panels, the input
# and every stage output rounded to the operand type (f32: the whole chain in f32) against the exact f64 chain, on the softmax maps
# P and the gradient maps dP' of these tests' own inputs at score scales 1, 4 and 35
# (tests/test_window_attention_bounds_cpu.py::test_filter_allowance_is_the_measured_one prints and re-checks it).  Figures: the
# largest rms over one row or one column of a map, relative to max |x| of that map, was 5.3e-4 (P) and 1.14e-3 (dP') in bf16,
# 2.8e-8 and 6.4e-8 in f32.  The bf16 figure is set by the roundings to bf16 and is the same on every host; the f32 one depends on the
# order in which the host's BLAS accumulates, so its constant is the next whole number of u above it, 2 u.  The margin of 2 is for
# what the emulation does not share with the kernel: the f32 product with the mask weights before the rounding of Y, and the order
# of accumulation.
ATTN_FILTER_RMS = {torch.bfloat16: 1.2e-3, torch.float32: 2 * U32}
ATTN_FILTER_MARGIN = 2.0
ATTN_FILTER_SIGMAS = 4.0          # with the margin: 8 measured standard deviations


def attn_other_band(lq, kt):
    """the kt-th band that is not lq (key tile kt of inter-band attention)"""
    return kt if kt < lq else kt + 1


def attn_key_slot(lq, lk):
    """which of the two key-gradient buffers (0: dk / dv, 1: dk2 / dv2) query band lq writes its gradient of key band lk to"""
    return lq if lq < lk else lq - 1


def attn_walk(nwin, chunks):
    """per = ceil(nwin / chunks) windows per workgroup; workgroup g walks [g * per, min(nwin, (g + 1) * per)).
    -> (per, busy workgroups, windows of the last busy one, idle workgroups)"""
    per = -(-nwin // chunks)
    busy = -(-nwin // per)
    return per, busy, nwin - (busy - 1) * per, chunks - busy


def attn2_chunks(nwin, heads, L, per_cu):
    """grid.x of attn2_* / attn2x_*: min(nwin, max(1, 256 * per_cu / (heads * L)))"""
    return min(nwin, max(1, 256 * per_cu // (heads * L)))


def attn1_bwd_chunks(nwin, heads, L):
    """grid.x of attn_bwd_kernel (v1): min(nwin, max(1, 1024 / (heads * L)))"""
    return min(nwin, max(1, 1024 // (heads * L)))


def attn_walks(nwin, heads, L, v1):
    """every (per, chunks) the backward of one problem may run with: the v1 kernel's one, or the v2 kernels' for per_cu 1 and 2"""
    cs = [attn1_bwd_chunks(nwin, heads, L)] if v1 else [attn2_chunks(nwin, heads, L, p) for p in (1, 2)]
    return [(attn_walk(nwin, c)[0], c) for c in cs]


def walk_crossings(nwin, chunks, nW):
    """image boundaries (first window of an image b > 0) that lie in the INTERIOR of some workgroup's range"""
    per = attn_walk(nwin, chunks)[0]
    return [w for w in range(nW, nwin, nW) if w % per != 0]


ATTN_MUTATIONS = ('bias_swapped', 'drop_key63', 'stale_coef', 'no_const', 'filter_09', 'dcoef_first_image', 'mask50')


class WAttnCase:
    """One window-attention problem: geometry and the storage-rounded operands, gathered into window order as f64.
    qkv [L*B*H*W, 3C] (q | k | v, image index = band * B + b), dout [L*B*H*W, C], tables [L*L, 225, heads] f32,
    coef [B, heads, 3] f32 or None.  qw / kw / vw / dow: [L, nwin, heads, 64, D]; window = (b * nWy + wy) * nWx + wx."""

    def __init__(self, dtype, D, heads, B, H, W, L, mode, shift, lfs, qkv, dout, tables, coef=None):
        self.dtype, self.D, self.heads, self.geo, self.lfs = dtype, D, heads, (B, H, W, L, mode, shift), lfs
        self.C, self.nkt, self.scale = D * heads, (1 if mode == 0 else L - 1), f32c(float(D) ** -0.5)
        self.nW = (H // 8) * (W // 8)
        self.nwin = B * self.nW
        self.qkv, self.dout, self.tables, self.coef = qkv, dout, tables, coef
        t = torch.arange(64)
        wy, wx = torch.arange(H // 8)[:, None, None], torch.arange(W // 8)[None, :, None]
        y, x = (wy * 8 + t // 8 + shift) % H, (wx * 8 + t % 8 + shift) % W                     # pixel of token t in the unrolled image
        img = torch.arange(L * B).view(L, B, 1, 1, 1)
        self.rows = ((img * H + y) * W + x).reshape(L, self.nwin, 64)
        g = lambda m, c0: m[self.rows][..., c0:c0 + self.C].double().view(L, self.nwin, 64, heads, D).transpose(2, 3)
        self.qw, self.kw, self.vw, self.dow = g(qkv, 0), g(qkv, self.C), g(qkv, 2 * self.C), g(dout, 0)
        i, j = t[:, None], t[None, :]
        self.bin = (i // 8 - j // 8 + 7) * 15 + (i % 8 - j % 8 + 7)                              # [64 queries][64 keys] -> 0 .. 224
        self.image = torch.arange(self.nwin) // self.nW
        # shift regions of the ROLLED image per axis: [0, size - 8), [size - 8, size - shift), [size - shift, size)
        reg = lambda p, size: (p >= size - 8).long() + (p >= size - shift).long()
        lab = (3 * reg(wy * 8 + t // 8, H) + reg(wx * 8 + t % 8, W)).reshape(self.nW, 64)
        self.diff = (lab[:, :, None] != lab[:, None, :]) if shift else torch.zeros(self.nW, 64, 64, dtype=torch.bool)

    def keys(self, lq):
        L, mode = self.geo[3], self.geo[4]
        return [lq] if mode == 0 else [attn_other_band(lq, kt) for kt in range(L - 1)]

    def gather(self, buf):
        """device or host [rows, >= C] buffer -> [L, nwin, heads, 64, D] f64 on the host (window order)"""
        L = self.geo[3]
        m = buf.detach().cpu()[:, :self.C]
        return m[self.rows].double().view(L, self.nwin, 64, self.heads, self.D).transpose(2, 3)


def attn_filter_f64():
    """-> (B1 as a function of f64 maps [..., 64, 64], |g| spectrum for abs_conv): the exact band filter of the 3-band decomposition"""
    from fwair import lfs
    panels, Mw = lfs.build_panels(lfs.band_masks_shifted('frequency_decompose_1', 0.5, 64, 64)[1].numpy())
    Mw = Mw.astype(np.float64)
    f = lambda x: torch.from_numpy(lfs.emulate_filter(x.numpy(), panels, Mw))
    delta = torch.zeros(64, 64, dtype=torch.float64)
    delta[0, 0] = 1.0
    return f, torch.fft.rfft2(f(delta).abs())


def attn_filter_emulated(dtype):
    """band_filter2 as the kernel of `dtype` runs it: panels in the operand type, the input and T, Y, Z rounded to it; f32: all in f32"""
    from fwair import lfs
    panels, Mw = lfs.build_panels(lfs.band_masks_shifted('frequency_decompose_1', 0.5, 64, 64)[1].numpy())
    if dtype == torch.bfloat16:
        panels = torch.from_numpy(panels).to(dtype).double().numpy()
        stage = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).double().numpy()
        return lambda x: torch.from_numpy(lfs.emulate_filter(x.double().numpy(), panels, Mw.astype(np.float64), stage)).to(x.dtype)
    panels = panels.astype(np.float32)
    return lambda x: torch.from_numpy(lfs.emulate_filter(x.float().numpy(), panels, Mw, lambda a: a.astype(np.float32))).to(x.dtype)


def abs_conv(t, ghat):
    """sum_(i', j') |g[i - i', j - j']| t[i', j'] (circular): what an element-wise error t of the filter's input can become behind it"""
    return torch.fft.irfft2(torch.fft.rfft2(t) * ghat, s=(64, 64)).clamp_min(0) * (1 + 1e-9)


def _attn_band(c, lq, ft, rs, filt, mutation, lse_in, walks):
    """Query band lq of case c evaluated in float type ft (f64: the reference; f32: the emulation), rs = the rounding of a value the
    kernel stores in the operand type.  -> dict of intermediates and results, all [nwin, heads, ...]."""
    B, H, W, L, mode, shift = c.geo
    keys, NK = c.keys(lq), 64 * c.nkt
    cat = lambda w, dim: torch.cat([w[lk] for lk in keys], dim).to(ft)
    q, k, v, do = c.qw[lq].to(ft), cat(c.kw, -2), cat(c.vw, -2), c.dow[lq].to(ft)
    bins = c.bin.t() if mutation == 'bias_swapped' else c.bin
    bias = torch.cat([c.tables[lq * L + lk].to(ft)[bins] for lk in keys], 1).permute(2, 0, 1)            # [heads, 64, NK]
    mval = -50.0 if mutation == 'mask50' else -100.0
    mask = (c.diff.to(ft) * mval).repeat(B, 1, c.nkt)[:, None]                                           # [nwin, 1, 64, NK]
    bm = bias + mask
    r = dict(q=q, k=k, v=v, do=do)
    s = (q @ k.transpose(-1, -2)) * c.scale + bm
    r['s'], r['smag'] = s, (q.abs() @ k.abs().transpose(-1, -2)) * c.scale + bias.abs() + mask.abs()
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    if mutation == 'drop_key63':
        e[..., NK - 1] = 0
    tot = e.sum(-1, keepdim=True)
    P = e * (1 / tot) if ft == torch.float32 else e / tot
    r['x'], r['tot'], r['lse'], r['P'] = s - m, tot, (m + torch.log(tot)).squeeze(-1), P
    one = torch.ones(c.nwin, c.heads, 1, 1, dtype=ft)
    ca, cb, cc = one, 0 * one, 0 * one
    if c.lfs:
        img = c.image.clone()
        if mutation == 'stale_coef':
            first = torch.arange(c.nW, c.nwin, c.nW)
            img[first] -= 1
        cf = c.coef.to(ft)[img]                                                                          # [nwin, heads, 3]
        ca, cb, cc = (cf[..., n, None, None] for n in range(3))
        if mutation == 'no_const':
            cb = 0 * cb
        if mutation == 'filter_09':
            cc = 0.9 * cc
    r['ca'], r['cb'], r['cc'] = ca, cb, cc

    def combine(p, tag):
        if not c.lfs:
            return p
        if c.lfs == 2:
            r['B1' + tag] = filt(p)
            return p * ca + cb + r['B1' + tag] * cc
        return p * ca + cb
    Pp = combine(P, 'f')
    r['Pp'] = Pp
    r['out'] = rs(rs(Pp) @ v)
    # ---- backward, from the lse the backward is given
    lse = (r['lse'] if lse_in is None else lse_in.to(ft))[..., None]
    Pb = torch.exp(s - lse)
    dPp = do @ v.transpose(-1, -2)
    Ppb = combine(Pb, 'b')
    r['xb'], r['Pb'], r['dPp'], r['Ppb'] = s - lse, Pb, dPp, Ppb
    dv = rs(rs(Ppb).transpose(-1, -2) @ do)
    if c.lfs == 2:
        r['B1d'] = filt(dPp)
        dP = dPp * ca + r['B1d'] * cc
    else:
        dP = dPp * ca
    if c.lfs:
        t3 = (r['B1d'] * Pb) if c.lfs == 2 else torch.zeros_like(Pb)
        r['cterms'] = torch.stack([dPp * Pb, dPp, t3], -1)                                               # [nwin, heads, 64, NK, 3]
        per_win = r['cterms'].sum((2, 3))
        credit = c.image.clone()
        if mutation == 'dcoef_first_image':
            per = walks[0][0]
            credit = c.image[torch.arange(c.nwin) // per * per]
        r['dcoef'] = torch.zeros(B, c.heads, 3, dtype=ft).index_add_(0, credit, per_win)
    Di = (Pb * dP).sum(-1, keepdim=True)
    dS = Pb * (dP - Di)
    r['dP'], r['Di'], r['dS'] = dP, Di, dS
    fold = lambda t: [torch.zeros(225, c.heads, dtype=t.dtype).index_add_(0, c.bin.reshape(-1), t[..., kt * 64:(kt + 1) * 64]
                      .sum(0).reshape(c.heads, 4096).t().contiguous()) for kt in range(c.nkt)]
    r['fold'] = fold
    r['dbias'] = fold(dS)
    dSs = rs(dS)
    r['dq'] = rs((dSs @ k) * c.scale)
    dk = rs((dSs.transpose(-1, -2) @ q) * c.scale)
    r['dk'], r['dv'] = list(dk.split(64, -2)), list(dv.split(64, -2))
    return r


def _attn_collect(c, bands):
    """per-band results -> out / dq [L, nwin, heads, 64, D], lse [L, nwin, heads, 64], dk / dv [L][kt] -> [nwin, heads, 64, D],
    dbias [L*L, 225, heads], dcoef [B, heads, 3] or None"""
    L = c.geo[3]
    res = {n: torch.stack([b[n] for b in bands]) for n in ('out', 'lse', 'dq')}
    res['dk'], res['dv'] = [b['dk'] for b in bands], [b['dv'] for b in bands]
    res['dbias'] = torch.zeros(L * L, 225, c.heads, dtype=bands[0]['dbias'][0].dtype)
    for lq, b in enumerate(bands):
        for kt, lk in enumerate(c.keys(lq)):
            res['dbias'][lq * L + lk] = b['dbias'][kt]
    res['dcoef'] = bands[0]['dcoef'] if c.lfs else None
    return res


def attn_emulate(c, lse_in=None):
    """The honest kernel on the host: f32 arithmetic, the operand type's rounding where the kernels round (P', dS, the outputs, the
    filter's stages), the backward fed with the emulated forward's own lse.  -> the results as _attn_collect returns them (f32)."""
    dt_ = c.dtype
    rs = (lambda t: t.to(dt_).to(torch.float32)) if dt_ != torch.float32 else (lambda t: t)
    filt = attn_filter_emulated(dt_) if c.lfs == 2 else None
    keep = ('out', 'lse', 'dq', 'dk', 'dv', 'dbias', 'dcoef')
    bands = []
    for lq in range(c.geo[3]):
        r = _attn_band(c, lq, torch.float32, rs, filt, None, None if lse_in is None else lse_in[lq], None)
        bands.append({n: r[n] for n in keep if n in r})
    return _attn_collect(c, bands)


def attn_reference(c, mutation=None, lse_in=None, v1=False):
    """f64 reference of case c (or of one of the wrong kernels of ATTN_MUTATIONS) with the element-wise bounds of a kernel's deviation
    from it.  lse_in [L, nwin, heads, 64]: the lse the backward is GIVEN (a kernel's own output); without it the backward bounds assume
    an lse within its own bound.  v1: attn_fwd / attn_bwd_kernel's walk instead of the v2 kernels'.
    -> {name: (value, tol)} shaped as _attn_collect returns them."""
    B, H, W, L, mode, shift = c.geo
    D, NK, u = c.D, 64 * c.nkt, U32
    ut = UBF if c.dtype == torch.bfloat16 else 0.0
    walks = attn_walks(c.nwin, c.heads, L, v1)
    filt, ghat = attn_filter_f64() if c.lfs == 2 else (None, None)
    fsig, Z = ATTN_FILTER_MARGIN * ATTN_FILTER_RMS[c.dtype], ATTN_FILTER_SIGMAS
    ident = lambda t: t
    stored = lambda val, tol: tol + ut * (val.abs() + tol)                      # a value rounded to the operand type
    vals, tols = [], []
    for lq in range(L):
        r = _attn_band(c, lq, torch.float64, ident, filt, mutation, None if lse_in is None else lse_in[lq].double(), walks)
        q, k, v, do, P, Pb = r['q'], r['k'], r['v'], r['do'], r['P'], r['Pb']
        ca, cb, cc = r['ca'], r['cb'], r['cc']
        t = {}
        es = (D + ATTN_SCORE_ROUNDINGS) * u * r['smag']
        # forward softmax: relative error of exp(x_j) is num_j; the error of the row maximum cancels between numerator and sum, the
        # sum's relative error is the P-weighted mean of num_j plus its own roundings
        num = es + ATTN_EXP_ARG_ROUNDINGS * u * r['x'].abs() + ATTN_EXP_VALUE_ERR
        avg = (P * num).sum(-1, keepdim=True)
        sum_err = avg + (NK // 4 + ATTN_SUM_EXTRA) * u
        tolP = P * torch.expm1(num + sum_err + ATTN_NORM_ERR) + F32_TINY
        lse = r['lse']
        t['lse'] = sum_err.squeeze(-1) + ATTN_LOG_ERR * (1 + torch.log(r['tot'].squeeze(-1))) + u * lse.abs()
        # backward softmax: exp(s - lse) with the given lse; without one, an lse within its bound
        e_lse = (u * lse.abs() if lse_in is not None else t['lse'])[..., None]
        tolPb = Pb * torch.expm1(es + e_lse + ATTN_EXP_ARG_ROUNDINGS * u * r['xb'].abs() + ATTN_EXP_VALUE_ERR) + F32_TINY
        tol_dPp = (D + ATTN_ACC_EXTRA) * u * (do.abs() @ v.abs().transpose(-1, -2))

        def filt_sigma(x):                                                     # rms of the filter's own error, per map
            return fsig * x.abs().amax((-1, -2), keepdim=True)

        def combine_tol(p, tolp, tag):                                         # error of P' = a p + b + c B1(p)
            if not c.lfs:
                return tolp
            tol = ca.abs() * tolp + ATTN_COMBINE_ROUNDINGS * u * ((ca * p).abs() + cb.abs())
            if c.lfs == 2:
                # the error of the filter's INPUT, carried through it exactly (|g| convolution); its own error goes separately
                tol = tol + cc.abs() * abs_conv(tolp, ghat) + ATTN_COMBINE_ROUNDINGS * u * (cc * r['B1' + tag]).abs()
            return tol
        zero = torch.zeros(c.nwin, c.heads, 1, 1, dtype=torch.float64)
        gP, gPb, gd = (cc.abs() * filt_sigma(x) if c.lfs == 2 else zero for x in (P, Pb, r['dPp']))     # sigma of c B1's own error
        tolPp = stored(r['Pp'], combine_tol(P, tolP, 'f'))
        out = r['Pp'] @ v
        t['out'] = stored(out, tolPp @ v.abs() + (NK + ATTN_ACC_EXTRA) * u * (r['Pp'].abs() @ v.abs())) \
            + Z * gP * (v * v).sum(-2, keepdim=True).sqrt()
        tolPpb = stored(r['Ppb'], combine_tol(Pb, tolPb, 'b'))
        dv = r['Ppb'].transpose(-1, -2) @ do
        t['dv'] = list((stored(dv, tolPpb.transpose(-1, -2) @ do.abs()
                               + (64 + ATTN_ACC_EXTRA) * u * (r['Ppb'].abs().transpose(-1, -2) @ do.abs()))
                        + Z * gPb * (do * do).sum(-2, keepdim=True).sqrt()).split(64, -2))
        dPp, dP = r['dPp'], r['dP']
        if c.lfs:
            tol_dP = ca.abs() * tol_dPp + 2 * u * (ca * dPp).abs()
            if c.lfs == 2:
                tB1d = abs_conv(tol_dPp, ghat)
                tol_dP = tol_dP + cc.abs() * tB1d + 2 * u * (cc * r['B1d']).abs()
                # <B1(dP'), P>: the filter's own error contracted with P over the whole map
                t3 = tB1d * Pb + (r['B1d'].abs() + tB1d) * tolPb + Z * filt_sigma(dPp) * (Pb * Pb).sum((-1, -2), keepdim=True).sqrt() / (64 * NK)
            else:
                t3 = torch.zeros_like(Pb)
            # d(a, b, c): per lane 16 products and sums per window, `per` windows, the wave fold, then one atomic per wave of
            # every workgroup that holds windows of the image
            chain = max(1 + ATTN_LANE_TERMS * c.nkt + per + ATTN_WAVE_FOLD + 4 * (-(-c.nW // per) + 1) for per, _ in walks)
            terr = torch.stack([tol_dPp * Pb + (dPp.abs() + tol_dPp) * tolPb, tol_dPp, t3], -1).sum((2, 3)) \
                + chain * u * r['cterms'].abs().sum((2, 3))
            t['dcoef'] = torch.zeros(B, c.heads, 3, dtype=torch.float64).index_add_(0, c.image, terr)
        else:
            tol_dP = tol_dPp
        Di = r['Di']
        tolD = (tolPb * dP.abs() + (Pb + tolPb) * tol_dP).sum(-1, keepdim=True) \
            + (1 + NK // 4 + ATTN_SUM_EXTRA) * u * (Pb * dP).abs().sum(-1, keepdim=True) \
            + Z * gd * (Pb * Pb).sum(-1, keepdim=True).sqrt()                   # c B1(dP')'s own error contracted with the row of P
        gS = Pb * gd                                                            # sigma of that error as dS = P (dP - D_i) carries it on
        dS = r['dS']
        tol_dS = tolPb * (dP - Di).abs() + (Pb + tolPb) * (tol_dP + tolD + u * (dP.abs() + Di.abs())) + ATTN_DS_ROUNDINGS * u * dS.abs()
        # dbias: `per` additions into the lane's accumulator, the LDS fold, one global atomic per busy workgroup
        bchain = max(per + ATTN_BIN_FOLD + attn_walk(c.nwin, ch)[1] for per, ch in walks)
        t['dbias'] = [a + bchain * u * b + Z * g.sqrt() for a, b, g in zip(r['fold'](tol_dS), r['fold'](dS.abs()), r['fold'](gS * gS))]
        tol_dSs = stored(dS, tol_dS)
        dq = (dS @ k) * c.scale
        t['dq'] = stored(dq, c.scale * (tol_dSs @ k.abs() + (NK + ATTN_ACC_EXTRA) * u * (dS.abs() @ k.abs()))) \
            + c.scale * Z * ((gS * gS) @ (k * k)).sqrt()
        dk = (dS.transpose(-1, -2) @ q) * c.scale
        t['dk'] = list((stored(dk, c.scale * (tol_dSs.transpose(-1, -2) @ q.abs()
                                              + (64 + ATTN_ACC_EXTRA) * u * (dS.abs().transpose(-1, -2) @ q.abs())))
                        + c.scale * Z * ((gS * gS).transpose(-1, -2) @ (q * q)).sqrt()).split(64, -2))
        vals.append(dict(out=out, lse=lse, dq=dq, dk=list(dk.split(64, -2)), dv=list(dv.split(64, -2)), dbias=r['dbias'],
                         dcoef=r.get('dcoef')))
        tols.append(t)
        del r
    V, T = _attn_collect(c, vals), _attn_collect(c, [dict(tt, dcoef=tt.get('dcoef')) for tt in tols])
    if c.lfs:
        T['dcoef'] = sum(tt['dcoef'] for tt in tols)
    return {n: (V[n], T[n]) for n in V if V[n] is not None}


def attn_with_prefill(ref, c, dbias0, dcoef0=None, v1=False):
    """the reference of a backward that ACCUMULATES into buffers holding dbias0 / dcoef0: value + pre-fill, and one more rounding of
    |pre-fill| for every atomic addition that lands on the word (one per busy workgroup for dbias; one per wave of every workgroup
    that holds windows of the image for dcoef)"""
    walks = attn_walks(c.nwin, c.heads, c.geo[3], v1)
    ref = dict(ref)
    badds = max(attn_walk(c.nwin, ch)[1] for _, ch in walks)
    ref['dbias'] = (ref['dbias'][0] + dbias0.double(), ref['dbias'][1] + badds * U32 * dbias0.double().abs())
    if dcoef0 is not None:
        adds = max(4 * (-(-c.nW // per) + 1) for per, _ in walks)
        ref['dcoef'] = (ref['dcoef'][0] + dcoef0.double(), ref['dcoef'][1] + adds * U32 * dcoef0.double().abs())
    return ref


def attn_outputs_flat(res):
    """{name: tensor or per-band lists} -> {name: one flat tensor} in a fixed order (dk / dv: [lq][kt] concatenated)"""
    flat = {}
    for n, x in res.items():
        if x is None:
            continue
        flat[n] = torch.cat([y.reshape(-1) for band in x for y in band]) if isinstance(x, list) else x.reshape(-1)
    return flat


def attn_inputs(dtype, D, heads, B, H, W, L, mode, shift, lfs, score_std=None, lam_scale=0.3, seed=0):
    """Seeded case: N(0, 1) operands rounded to `dtype`; with score_std, q and k are scaled so that scale * q.k has that standard
    deviation (sigma_q = sigma_k = sqrt(score_std)); tables 0.5 N(0, 1); lambda = lam_scale N(0, 1) per (image, band, head), turned
    into (a, b, c) = (1 + l2, -l2 / 64, l1 - l2) (lfs 2) or (1 + l1, -l1 / 64, 0) (lfs 1) in f32."""
    g = torch.Generator().manual_seed(seed * 7919 + 31 * D + 17 * heads + B * H * W + 5 * L + mode + shift + lfs)
    C, rows = D * heads, L * B * H * W
    qkv = torch.randn(rows, 3 * C, generator=g)
    if score_std:
        qkv[:, :2 * C] *= score_std ** 0.5
    dout = torch.randn(rows, C, generator=g)
    tables = 0.5 * torch.randn(L * L, 225, heads, generator=g)
    coef = None
    if lfs:
        lam = lam_scale * torch.randn(B, 2, heads, generator=g)
        l1, l2 = (lam[:, 0], lam[:, 1]) if lfs == 2 else (torch.zeros_like(lam[:, 0]), lam[:, 0])
        coef = torch.stack([1 + l2, -l2 / 64, (l1 - l2) if lfs == 2 else torch.zeros_like(l1)], -1).float().contiguous()
    r = lambda t: t.to(dtype).float()
    return WAttnCase(dtype, D, heads, B, H, W, L, mode, shift, lfs, r(qkv), r(dout), tables, coef)


# ------------------------------------------------------------------------------------------------ convolutional plug-ins (csrc/fw_conv.hip)
# Plain f64 statements of the 15 entries, written from include/fwair.h and the reference operators (nn.Conv2d, nn.BatchNorm2d, the
# published DCNv2 definition), with element-wise bounds counted from the kernels' roundings.  Every statement is a function of a float
# type `ft` and a storage rounding `rs`: ft = f64, rs = identity is the reference; ft = f32 with rs = the operand type's rounding is
# the honest emulation tests/test_conv_bounds_cpu.py holds against the bounds; `mutation` names one of the wrong kernels the bounds
# must reject.  Nothing here imports fwair.convnets.
CONV_MUTATIONS = ('taps_not_flipped', 'halo_shift', 'border_clamped', 'bias_after_act', 'res_before_act', 'cin1_off_group',
                  'stride2_at_2o')
BN_MUTATIONS = ('biased_running_var', 'rstd_no_eps', 'dres_before_slope')
DCN_MUTATIONS = ('validity_ignored', 'mask_no_sigmoid_grad', 'offsets_swapped')


def rup(v, m):
    return (v + m - 1) // m * m


def conv_chunk(dtype):
    """elements of one 64-byte MFMA K chunk"""
    return 32 if dtype == torch.bfloat16 else 16


def storage_rounding(dtype):
    """rs(t): t rounded to `dtype` (round to nearest even), in t's own float type"""
    return (lambda t: t) if dtype in (torch.float32, torch.float64) else (lambda t: t.to(dtype).to(t.dtype))


def conv_out_size(n, stride):
    return (n - 1) // stride + 1


def conv_panel_ref(weight, cin, kind='fwd', flip=True):
    """weight [Co, Ci, k, k] (k = 1 | 3) -> the tap-major panel fw_conv3x3 reads, in weight's float type.
    'fwd':   [roundup(Co, 16)][9 * cin], element (co, tap, ci); a 1x1 weight sits at the centre tap; cin >= Ci, zero beyond Ci.
    'dgrad': [roundup(Ci, 16)][9 * cin], element (ci, 8 - tap, co); cin >= Co.  The input gradient of a stride-1 convolution is the
             convolution of dy with this panel.  flip=False leaves the taps unflipped (a mutation).
    Rows above Co (Ci) are zero."""
    Co, Ci, k, _ = weight.shape
    if kind == 'fwd':
        out = torch.zeros(rup(Co, 16), 9, cin, dtype=weight.dtype)
        if k == 3:
            out[:Co, :, :Ci] = weight.reshape(Co, Ci, 9).transpose(1, 2)
        else:
            out[:Co, 4, :Ci] = weight.reshape(Co, Ci)
    else:
        assert k == 3
        out = torch.zeros(rup(Ci, 16), 9, cin, dtype=weight.dtype)
        w = weight.reshape(Co, Ci, 9).permute(1, 2, 0)                    # (ci, tap, co)
        out[:Ci, :, :Co] = w.flip(1) if flip else w
    return out.reshape(out.shape[0], 9 * cin)


def _tap_rows(B, H, W, S, oy_shift=0, ix_shift=0):
    """-> (rows [B*Ho*Wo, 9] clamped source row of every tap, ok [B*Ho*Wo, 9] inside the image): iy = oy*S - 1 + ky, ix = ox*S - 1 + kx"""
    Ho, Wo = conv_out_size(H, S), conv_out_size(W, S)
    tap = torch.arange(9)
    iy = (torch.arange(Ho) * S - 1 + oy_shift)[:, None, None] + (tap // 3)[None, None, :]
    ix = (torch.arange(Wo) * S - 1 + ix_shift)[None, :, None] + (tap % 3)[None, None, :]
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    row = iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)
    rows = (torch.arange(B)[:, None, None, None] * (H * W) + row[None]).reshape(-1, 9)
    return rows, ok[None].expand(B, Ho, Wo, 9).reshape(-1, 9)


def im2col3_ref(x, B, H, W, C, stride, mutation=None):
    """x [B*H*W, >= C] -> col [B*Ho*Wo, 9 * C]: col[(b, oy, ox)][tap * C + c] = x[(b, oy*S - 1 + ky, ox*S - 1 + kx)][c], 0 outside the
    image (pad columns of x are never read).  A data mover: exact in every type."""
    s = 1 if mutation == 'stride2_at_2o' else 0                            # both axes read S o .. S o + 2 in place of S o - 1 .. S o + 1
    rows, ok = _tap_rows(B, H, W, stride, oy_shift=s, ix_shift=s + (1 if mutation == 'halo_shift' else 0))
    col = x[:, :C][rows]                                                   # [Mo, 9, C]
    if mutation != 'border_clamped':
        col = torch.where(ok[..., None], col, torch.zeros((), dtype=col.dtype))
    return col.reshape(rows.shape[0], 9 * C)


def col2im3_ref(dcol, B, H, W, C, stride):
    """the adjoint of im2col3_ref: dx[(b, y, x)][c] = sum of dcol[(b, oy, ox)][tap * C + c] over the (oy, ox, tap) that read (y, x).
    -> (dx [B*H*W, C], mag = the same sum of magnitudes) in dcol's type"""
    rows, ok = _tap_rows(B, H, W, stride)
    d = dcol.reshape(-1, 9, C) * ok[..., None].to(dcol.dtype)
    dx = torch.zeros(B * H * W, C, dtype=dcol.dtype).index_add_(0, rows.reshape(-1), d.reshape(-1, C))
    mag = torch.zeros(B * H * W, C, dtype=dcol.dtype).index_add_(0, rows.reshape(-1), d.abs().reshape(-1, C))
    return dx, mag


COL2IM_ROUNDINGS = 9              # at most 9 taps land on one pixel: 8 additions, and one spare


def col2im3_bound(dx, mag, dtype):
    tol = COL2IM_ROUNDINGS * U32 * mag
    return tol + UBF * (dx.abs() + tol) if dtype == torch.bfloat16 else tol


def popcount(v):
    return bin(v).count('1')


CONV_LRELU_ROUNDINGS = 1          # x * slope


def conv3x3_ref(x, x2, cin, cin1, panel, bias, res, cout, B, H, W, stride, taps, act, slope, out_dtype, ft=torch.float64,
                mutation=None):
    """fw_conv3x3 in float type ft.  x [B*H*W, >= cin1], x2 [B*H*W, >= cin - cin1] or None (channels [0, cin1) from x, the rest from
    x2), panel [roundup(cout, 16), 9 * cin] (conv_panel_ref), bias [cout] f32 or None, res [Mo, >= cout] or None; order: + bias,
    LeakyReLU (act 1), + res.  out_dtype: the type the output is STORED in.
    -> (value [Mo, cout], tol [Mo, cout]).  The bound is the GEMM bound (GemmRef on the f64 im2col operand, K = popcount(taps) * cin,
    plus GEMM_EPI_ROUNDINGS for the epilogue), carried through LeakyReLU (Lipschitz max(1, |slope|), one product) and the storage
    rounding; the f32 emulation passes tol = None."""
    split = cin1 + (64 if mutation == 'cin1_off_group' else 0)           # the mutation switches sources one 64-channel group late
    assert x2 is None or x.shape[1] >= split
    src = x[:, :cin].to(ft) if x2 is None else torch.cat([x[:, :split], x2[:, split - cin1:cin - cin1]], 1).to(ft)
    mask = torch.tensor([(taps >> t) & 1 for t in range(9)], dtype=ft).repeat_interleave(cin)
    w = panel[:cout].to(ft) * mask
    K = popcount(taps & 0x1ff) * cin
    M1, Mo1 = H * W, conv_out_size(H, stride) * conv_out_size(W, stride)
    vals, tols = [], []
    for b in range(B):                                                     # one image at a time keeps the operand small
        col = im2col3_ref(src[b * M1:(b + 1) * M1], 1, H, W, cin, stride, mutation)
        ref = GemmRef(col, w)
        v, mag = ref.acc, ref.mag
        r = res[b * Mo1:(b + 1) * Mo1, :cout].to(ft) if res is not None else None
        bv = bias.to(ft) if bias is not None else None
        if bv is not None and mutation != 'bias_after_act':
            v, mag = v + bv, mag + bv.abs()
        if r is not None and mutation == 'res_before_act':
            v = v + r
        tol = (K + GEMM_EPI_ROUNDINGS) * U32 * mag
        if act == 1:
            tol = max(1.0, abs(slope)) * tol + CONV_LRELU_ROUNDINGS * U32 * v.abs()
            v = torch.where(v > 0, v, v * f32c(slope))
        if bv is not None and mutation == 'bias_after_act':
            v = v + bv
        if r is not None and mutation != 'res_before_act':
            v, tol = v + r, tol + (K + GEMM_EPI_ROUNDINGS) * U32 * r.abs()
        if out_dtype == torch.bfloat16:
            tol = tol + UBF * (v.abs() + tol)
        vals.append(v); tols.append(tol)
    v = torch.cat(vals)
    return (v, torch.cat(tols)) if ft == torch.float64 else (storage_rounding(out_dtype)(v), None)


# ---- DCNv2 (fw_dcn_im2col / fw_dcn_bwd).  om [M, 32] f32: 2k / 2k + 1 = (dy, dx) of tap k, 18 + k = mask logit, 27..31 unused.
# The kernels form the sample point in f32: py = float(y + ky - 1) + dy is ONE f32 addition of an exact integer and the stored offset,
# and the reference takes exactly that f32 value (the statement is "at the stored inputs"); floor and the fractions wy = py - floor(py)
# are then exact.  What is left to count, per term w * a * m of the sample:
#   1 - wy, 1 - wx (one rounding each), their product, the product with the pixel, the sum of the four corners (3), the product with m
DCN_TERM_ROUNDINGS = 8
# m = 1 / (1 + __expf(-o)): the exp argument (product with log2 e and its f32 value: relative 3 u |o| of the result), v_exp_f32 1 ulp,
# the sum 1 + e, the division (1 ulp); e / (1 + e) <= 1 scales the first two
DCN_SIGMOID_ROUNDINGS = 3         # 1 + e, the division (2 u)
DCN_WAVE_FOLD = 6


def dcn_sigmoid_err(o):
    """relative error of the kernels' sigmoid(o), o an f64 tensor of f32 logits"""
    return ATTN_EXP_ARG_ROUNDINGS * U32 * o.abs() + ATTN_EXP_VALUE_ERR + DCN_SIGMOID_ROUNDINGS * U32


def _dcn_geometry(om, B, H, W, ft, mutation=None):
    """per tap k: dict(rows [4][M] clamped corner rows (00, 01, 10, 11), valid [4][M], wy, wx [M] in ft, m [M] in ft)"""
    M = B * H * W
    p = torch.arange(M)
    xx, yy, b0 = p % W, (p // W) % H, (p // (W * H)) * (H * W)
    o32 = om.float()
    taps = []
    for k in range(9):
        iy, ix = (2 * k + 1, 2 * k) if mutation == 'offsets_swapped' else (2 * k, 2 * k + 1)
        py = (yy + (k // 3 - 1)).float() + o32[:, iy]                      # the kernel's single f32 addition
        px = (xx + (k % 3 - 1)).float() + o32[:, ix]
        fy, fx = py.floor(), px.floor()
        wy, wx = (py - fy).to(ft), (px - fx).to(ft)                        # exact in f32
        y0, x0 = fy.long(), fx.long()
        vy = [(y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)]
        vx = [(x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)]
        cy = [y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)]
        cx = [x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)]
        rows = [b0 + cy[i] * W + cx[j] for i in (0, 1) for j in (0, 1)]
        valid = [vy[i] & vx[j] for i in (0, 1) for j in (0, 1)]
        if mutation == 'validity_ignored':
            valid = [torch.ones_like(v) for v in valid]
        logit = om[:, 18 + k].to(ft)
        m = 1 / (1 + torch.exp(-logit))
        taps.append(dict(rows=rows, valid=valid, wy=wy, wx=wx, m=m, logit=om[:, 18 + k].double()))
    return taps


def _dcn_weights(t):
    wy, wx = t['wy'], t['wx']
    return [(1 - wy) * (1 - wx), (1 - wy) * wx, wy * (1 - wx), wy * wx]


def dcn_im2col_ref(x, om, B, H, W, C, out_dtype, ft=torch.float64, mutation=None):
    """col[p][k * C + c] = sigmoid(om[p][18 + k]) * sum over the four corners of w_corner * x[corner][c], a corner outside the image
    counting as zero.  x [M, >= C] storage-rounded values, om [M, 32] f32.  -> (col [M, 9 * C], tol); f32 emulation: tol = None."""
    xs = x[:, :C].to(ft)
    cols, tols = [], []
    for t in _dcn_geometry(om, B, H, W, ft, mutation):
        s, mag = 0, 0
        for w, r, v in zip(_dcn_weights(t), t['rows'], t['valid']):
            term = torch.where(v[:, None], w[:, None] * xs[r], torch.zeros((), dtype=ft))
            s, mag = s + term, mag + term.abs()
        m = t['m'][:, None]
        v = s * m
        tol = (DCN_TERM_ROUNDINGS * U32 + dcn_sigmoid_err(t['logit'])[:, None].to(ft)) * mag * m
        if out_dtype == torch.bfloat16:
            tol = tol + UBF * (v.abs() + tol)
        cols.append(v); tols.append(tol)
    col = torch.cat(cols, 1)
    return (col, torch.cat(tols, 1)) if ft == torch.float64 else (storage_rounding(out_dtype)(col), None)


def dcn_bwd_ref(dcol, x, om, B, H, W, C, dx0=None, ft=torch.float64, mutation=None):
    """the backward of dcn_im2col_ref from g = dcol [M, 9 * C]:
      dx[corner][c] += g m w_corner (valid corners only; a scatter, f32 atomics in the kernel), on top of dx0 [M, C]
      dom[p][2k] = sum_c g m ((1 - wx)(a10 - a00) + wx (a11 - a01)),  dom[p][2k + 1] likewise in x,
      dom[p][18 + k] = (sum_c g val) m (1 - m);  a = the corner values, zero where invalid;  columns 27..31 are not written.
    -> dict dx, dom [M, 27] with tol_dx, tol_dom (f64) or just dx, dom (emulation)"""
    M = B * H * W
    xs, g = x[:, :C].to(ft), dcol.to(ft).reshape(M, 9, C)
    dx = torch.zeros(M, C, dtype=ft) if dx0 is None else dx0.to(ft).clone()
    dxmag, adds = dx.abs().clone(), torch.zeros(M, dtype=ft)
    dxrel = torch.zeros(M, C, dtype=ft)                                    # sum of |term| * the term's own relative error
    dom, tdom = torch.zeros(M, 27, dtype=ft), torch.zeros(M, 27, dtype=ft)
    chain = -(-C // 64) + DCN_WAVE_FOLD
    for k, t in enumerate(_dcn_geometry(om, B, H, W, ft, mutation)):
        gk, m, wy, wx = g[:, k], t['m'][:, None], t['wy'][:, None], t['wx'][:, None]
        em = dcn_sigmoid_err(t['logit'])[:, None].to(ft)
        a = [torch.where(v[:, None], xs[r], torch.zeros((), dtype=ft)) for r, v in zip(t['rows'], t['valid'])]
        for w, r, v in zip(_dcn_weights(t), t['rows'], t['valid']):
            term = torch.where(v[:, None], gk * m * w[:, None], torch.zeros((), dtype=ft))
            dx.index_add_(0, r, term)
            dxmag.index_add_(0, r, term.abs())
            dxrel.index_add_(0, r, term.abs() * (6 * U32 + em))            # g m, 1 - wy, 1 - wx, two products, and one spare
            adds.index_add_(0, r, v.to(ft))
        val = (1 - wy) * ((1 - wx) * a[0] + wx * a[1]) + wy * ((1 - wx) * a[2] + wx * a[3])
        vmag = (1 - wy) * ((1 - wx) * a[0].abs() + wx * a[1].abs()) + wy * ((1 - wx) * a[2].abs() + wx * a[3].abs())
        gy = (1 - wx) * (a[2] - a[0]) + wx * (a[3] - a[1])
        gymag = (1 - wx) * (a[2].abs() + a[0].abs()) + wx * (a[3].abs() + a[1].abs())
        gx = (1 - wy) * (a[1] - a[0]) + wy * (a[3] - a[2])
        gxmag = (1 - wy) * (a[1].abs() + a[0].abs()) + wy * (a[3].abs() + a[2].abs())
        sm, smag = (gk * val).sum(1), (gk.abs() * vmag).sum(1)
        m1, e1 = t['m'], em[:, 0]
        dom[:, 2 * k], dom[:, 2 * k + 1] = (gk * m * gy).sum(1), (gk * m * gx).sum(1)
        if mutation == 'mask_no_sigmoid_grad':
            dom[:, 18 + k] = sm
        else:
            dom[:, 18 + k] = sm * m1 * (1 - m1)
        per = (DCN_TERM_ROUNDINGS + chain) * U32
        tdom[:, 2 * k] = (per + e1) * (gk.abs() * m * gymag).sum(1)
        tdom[:, 2 * k + 1] = (per + e1) * (gk.abs() * m * gxmag).sum(1)
        # m (1 - m): |dm| = m e1; 1.0f - m carries |dm| and its own rounding ABSOLUTELY (m next to 1 loses 1 - m altogether)
        dm = m1 * e1
        d1m = dm + U32 * (1 - m1) + U32 * m1
        tdom[:, 18 + k] = per * smag * m1 * (1 - m1) + smag * (dm * (1 - m1) + m1 * d1m + 2 * U32 * m1 * (1 - m1))
    if ft != torch.float64:
        return dict(dx=dx, dom=dom)
    tol_dx = dxrel + (adds[:, None] + 1) * U32 * dxmag
    return dict(dx=dx, dom=dom, tol_dx=tol_dx, tol_dom=tdom, adds=adds)


# ---- BatchNorm2d on a token-major map (fw_bn_cl_fwd / fw_bn_cl_bwd).  The kernels take the batch variance in ONE pass,
#     var = E[x^2] - mean^2 from f32 column sums,
# so the error of the two sums, each relative to its own magnitude, lands on var relative to E[x^2] = var (1 + mean^2 / var): the
# conditioning factor BN_COND below, stated in the bound explicitly.  The reference takes mean and variance in two passes in f64.
# Column sums: a thread adds ceil(rows / (grid * RL)) values, then one atomic per thread lands on the word: grid * RL of them.
BN_MEAN_ROUNDINGS = 1             # sum / rows
BN_VAR_ROUNDINGS = 7              # x * x, the division, mean * mean, the difference, and E|x| |mean| <= E[x^2] taken twice for d(mean^2)
RSQRT_ERR = 2 * U32               # rsqrtf: 1 ulp
BN_APPLY_ROUNDINGS = 5            # x - mean, * rstd, * gamma, + beta, + res
BN_BWD_ROUNDINGS = 8              # dz * slope, x - mean, * rstd (xh), gamma * rstd, 1 / rows, two products, two differences (fma halves them)


def bn_grid(rows, C):
    """-> (blocks, RL): the launch of colstats_kernel / bn_bwd_stats_kernel by the contract of fw_bn_cl_*"""
    RL = max(256 // (C // 4), 1)
    return min(-(-rows // RL), 1024), RL


def bn_chain(rows, C):
    """longest chain of f32 additions between one value and its column sum"""
    grid, RL = bn_grid(rows, C)
    lanes = min(rows, grid * RL)
    return -(-rows // lanes) + lanes


def bn_cond(mean, var):
    """1 + mean^2 / var (inf where var == 0)"""
    return 1 + mean * mean / var


def bn_cl_fwd_ref(x, gamma, beta, rmean, rvar, res, C, training, eps, momentum, slope, out_dtype, ft=torch.float64, mutation=None):
    """x [rows, >= C] storage-rounded, gamma / beta / rmean / rvar [C] f32, res [rows, >= C] or None.
    y = lrelu((x - mean) rstd gamma + beta [+ res], slope) (slope 1.0: no activation); train: batch statistics (two passes in f64),
    running statistics r' = r (1 - momentum) + momentum s with the UNBIASED variance rows / max(rows - 1, 1); eval: running statistics.
    -> dict y, mean, rstd, rmean, rvar [, tol_*] (f64), or the f32 emulation's values (one-pass variance, as the kernel)."""
    rows = x.shape[0]
    xs = x[:, :C].to(ft)
    eps, momentum, slope = f32c(eps), f32c(momentum), f32c(slope)
    g, b, rm, rv = (t.to(ft) for t in (gamma, beta, rmean, rvar))
    emul = ft != torch.float64
    out = {}
    if training:
        if emul:
            mean = xs.sum(0) / rows
            var = ((xs * xs).sum(0) / rows - mean * mean).clamp_min(0)
        else:
            mean = xs.mean(0)
            var = ((xs - mean) ** 2).mean(0)
        unb = 1.0 if mutation == 'biased_running_var' else rows / max(rows - 1, 1)
        rstd = 1 / (var.sqrt() if mutation == 'rstd_no_eps' else (var + eps).sqrt())
        out['rmean'], out['rvar'] = rm * (1 - momentum) + momentum * mean, rv * (1 - momentum) + momentum * var * unb
        if not emul:
            chain = bn_chain(rows, C)
            cond = bn_cond(mean, var)
            ex2 = torch.where(var > 0, var * cond, mean * mean)             # E[x^2] = var (1 + mean^2 / var)
            e_mean = (chain + BN_MEAN_ROUNDINGS) * U32 * xs.abs().mean(0)
            e_var = (3 * chain + BN_VAR_ROUNDINGS) * U32 * ex2
            hi, lo = 1 / ((var - e_var).clamp_min(0) + eps).sqrt(), 1 / (var + e_var + eps).sqrt()
            e_rstd = torch.maximum(hi - rstd, rstd - lo) + (U32 + RSQRT_ERR) * hi
            out['tol_rmean'] = momentum * e_mean + 3 * U32 * ((rm * (1 - momentum)).abs() + (momentum * mean).abs())
            out['tol_rvar'] = momentum * unb * e_var + 5 * U32 * ((rv * (1 - momentum)).abs() + momentum * var * unb)
            out['cond'] = cond
    else:
        mean, var = rm, rv
        rstd = 1 / (var + eps).sqrt()
        out['rmean'], out['rvar'] = rm, rv
        if not emul:
            e_mean, e_rstd = torch.zeros_like(mean), (U32 + RSQRT_ERR) * rstd
            out['tol_rmean'] = out['tol_rvar'] = torch.zeros_like(mean)
    d = xs - mean
    t = d * rstd * g
    v = t + b
    r = res[:, :C].to(ft) if res is not None else None
    if r is not None:
        v = v + r
    y = torch.where(v > 0, v, v * slope)
    out.update(y=y, mean=mean, rstd=rstd)
    if emul:
        out['y'] = storage_rounding(out_dtype)(y)
        return out
    tol = g.abs() * (d.abs() * e_rstd + (rstd + e_rstd) * e_mean) \
        + BN_APPLY_ROUNDINGS * U32 * (t.abs() + b.abs() + (r.abs() if r is not None else 0))
    tol = max(1.0, abs(slope)) * tol + U32 * v.abs()
    out['tol_y'] = tol + UBF * (y.abs() + tol) if out_dtype == torch.bfloat16 else tol
    out['tol_mean'], out['tol_rstd'] = e_mean + U32 * mean.abs(), e_rstd
    return out


def bn_cl_bwd_ref(dy, y, x, mean, rstd, gamma, C, training, slope, out_dtype, ft=torch.float64, mutation=None):
    """dz = dy * (slope where y < 0) (slope 1.0: dz = dy, y is not read); s0 = sum dz = d(beta), s1 = sum dz xh = d(gamma),
    xh = (x - mean) rstd with the GIVEN mean / rstd [C] (f32 values); dx = gamma rstd (dz - s0 / rows - xh s1 / rows) (train) or
    gamma rstd dz (eval); dres = dz.  -> dict dx, dres, sums [2, C] [, tol_*]"""
    rows = x.shape[0]
    slope = f32c(slope)
    dz = dy[:, :C].to(ft)
    if slope != 1.0:
        dz = torch.where(y[:, :C].to(ft) < 0, dz * slope, dz)
    mean, rstd, g = mean.to(ft), rstd.to(ft), gamma.to(ft)
    xh = (x[:, :C].to(ft) - mean) * rstd
    s0, s1 = dz.sum(0), (dz * xh).sum(0)
    gr = g * rstd
    dx = gr * (dz - s0 / rows - xh * s1 / rows) if training else gr * dz
    rs = storage_rounding(out_dtype)
    dres = dy[:, :C].to(ft) if mutation == 'dres_before_slope' else dz
    if ft != torch.float64:
        return dict(dx=rs(dx), dres=rs(dres), sums=torch.stack([s0, s1]))
    chain = bn_chain(rows, C)
    t0, t1 = (chain + 1) * U32 * dz.abs().sum(0), (chain + 4) * U32 * (dz * xh).abs().sum(0)
    mag = dz.abs() + (s0 / rows).abs() + (xh * s1 / rows).abs() if training else dz.abs()
    tol = gr.abs() * ((t0 + xh.abs() * t1) / rows if training else 0) + BN_BWD_ROUNDINGS * U32 * gr.abs() * mag
    st = (lambda v, t: t + UBF * (v.abs() + t)) if out_dtype == torch.bfloat16 else (lambda v, t: t)
    return dict(dx=dx, dres=dres, sums=torch.stack([s0, s1]), tol_dx=st(dx, tol), tol_dres=st(dres, U32 * dz.abs()),
                tol_sums=torch.stack([t0, t1]))


# ---- the elementwise entries: one f32 expression per element, stored in the operand type
def lrelu_ref(x, slope):
    return torch.where(x > 0, x, x * f32c(slope))


def lrelu_bwd_ref(dy, y, slope):
    """from the OUTPUT's sign"""
    return torch.where(y < 0, dy * f32c(slope), dy)


def dgm_fwd_ref(x, dcn, gamma, beta, slope):
    """-> (out, tol before the storage rounding): lrelu(x + dcn + x gamma + beta); four f32 operations on terms of these magnitudes"""
    v = x + dcn + x * gamma + beta
    return lrelu_ref(v, slope), 4 * U32 * (x.abs() + dcn.abs() + (x * gamma).abs() + beta.abs()) * max(1.0, abs(slope))


def dgm_bwd_ref(dout, out, x, gamma, slope):
    """-> dict dz, dx, dgamma and tol_* (before the storage rounding)"""
    dz = torch.where(out < 0, dout * f32c(slope), dout)
    dx, dg = dz * (1 + gamma), dz * x
    return dict(dz=dz, dx=dx, dgamma=dg, tol_dz=U32 * dz.abs(), tol_dx=3 * U32 * dz.abs() * (1 + gamma.abs()), tol_dgamma=2 * U32 * dg.abs())


def gap_cl_ref(x, B, P, C):
    """[B * P, >= C] -> (mean over the P pixels [B, C], tol: P sequential f32 additions and the division)"""
    v = x[:, :C].reshape(B, P, C)
    return v.mean(1), (P + 1) * U32 * v.abs().mean(1)


def gap_cl_bwd_ref(dgap, P):
    """[B, C] -> [B * P, C]: dgap / P broadcast (one f32 division)"""
    return (dgap / P).repeat_interleave(P, 0)


def nchw_to_tokens_ref(img, Cp):
    """f32 [B, Ci, HW] -> [B * HW, Cp], channels >= Ci zero"""
    B, Ci, HW = img.shape
    out = torch.zeros(B * HW, Cp, dtype=img.dtype)
    out[:, :Ci] = img.permute(0, 2, 1).reshape(B * HW, Ci)
    return out


def tokens_to_nchw_ref(tok, B, Ci, HW):
    return tok[:, :Ci].reshape(B, HW, Ci).permute(0, 2, 1).contiguous()


def stored(value, tol, dtype):
    """bound of a value after its rounding to the storage type"""
    return tol + UBF * (value.abs() + tol) if dtype == torch.bfloat16 else tol + U32 * value.abs()


# ---- seeded cases shared by tests/test_conv_bounds_cpu.py (host) and tests/test_conv_kernels_gpu.py (device)
def dyadic(*shape, seed, lo, hi, denom):
    """integers in [lo, hi] over denom (a power of two): sums of a few thousand of them are exact in f32, in any order"""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float() / denom


def padded(values, ld, pad=float('nan')):
    """[rows, C] -> [rows, ld] with `pad` in the columns >= C"""
    out = torch.full((values.shape[0], ld), pad, dtype=values.dtype)
    out[:, :values.shape[1]] = values
    return out


class ConvCase:
    """One fw_conv3x3 problem.  Operands are f32 tensors holding values already rounded to `dtype`; x / x2 / res carry `pad` in the
    columns the kernel must not consume.  exact: x, res, bias = integers / 8, weights = small integers, slope 1/8, so every f32
    partial sum is exact and the result does not depend on the order of summation.  dgrad: the operand is dy [M, cin] of a stride-1
    convolution with weight [cin, cout, 3, 3] and the panel is the flipped, transposed one: the output is dx [M, cout]."""

    def __init__(self, dtype, B, H, W, stride, cin, cout, k=3, cin1=None, bias=True, act=1, slope=0.1, res=True, out_f32=False,
                 ldx=None, ldx2=None, ldr=None, ldo=None, pad=float('nan'), seed=0, dgrad=False, exact=False, flip=True):
        self.dtype, self.geo, self.stride, self.cin, self.cout = dtype, (B, H, W), stride, cin, cout
        self.cin1 = cin if cin1 is None else cin1
        self.taps, self.act, self.slope = (0x1ff if k == 3 else 0x010), act, (0.125 if exact else slope)
        self.out_dtype = torch.float32 if out_f32 or dtype == torch.float32 else dtype
        self.out_f32 = int(out_f32)
        self.Ho, self.Wo = conv_out_size(H, stride), conv_out_size(W, stride)
        M, Mo = B * H * W, B * self.Ho * self.Wo
        rs = storage_rounding(dtype)
        s = 1000 * seed + 7 * cin + cout + H * W
        if exact:
            mk = lambda *sh, n: dyadic(*sh, seed=s + n, lo=-8, hi=8, denom=8)
            wgt = dyadic(*((cin, cout) if dgrad else (cout, cin)), k, k, seed=s + 9, lo=-2, hi=2, denom=1)
        else:
            mk = lambda *sh, n: rs(signed_magnitudes(*sh, seed=s + n))
            wgt = rs(signed_magnitudes(*((cin, cout) if dgrad else (cout, cin)), k, k, seed=s + 9))
        xs = mk(M, cin, n=1)
        self.x = padded(xs[:, :self.cin1], ldx or self.cin1, pad)
        self.x2 = padded(xs[:, self.cin1:], ldx2 or cin - self.cin1, pad) if self.cin1 < cin else None
        self.weight = wgt
        self.panel = conv_panel_ref(wgt, cin, 'dgrad' if dgrad else 'fwd', flip)
        self.bias = (mk(cout, n=2) if exact else signed_magnitudes(cout, seed=s + 2)) if bias else None
        self.res = padded(mk(Mo, cout, n=3), ldr or cout, pad) if res else None
        self.ldo = ldo or cout

    def ref(self, ft=torch.float64, mutation=None):
        B, H, W = self.geo
        return conv3x3_ref(self.x, self.x2, self.cin, self.cin1, self.panel, self.bias, self.res, self.cout, B, H, W, self.stride,
                           self.taps, self.act, self.slope, self.out_dtype, ft, mutation)

    def tiles(self):
        """output tiles of 4 x 16 pixels = workgroups asked for (the grid is capped at CONV_GRID_CAP)"""
        return self.geo[0] * (-(-self.Ho // 4)) * (-(-self.Wo // 16))


CONV_GRID_CAP = 2048
BN_GRID_CAP = 1024
DCN_BWD_GRID_CAP = 65536          # blocks of 4 waves, one (pixel, tap) per wave and trip


def bn_inputs(dtype, rows, C, ratio=0.0, std=0.0625, seed=0, exact=False):
    """-> dict x, res, dy [rows, C] (rounded to dtype), gamma, beta, rmean, rvar [C] f32.  Columns have |mean| / std = ratio.
    exact: integers / 8 in [-1, 1], so sums of x and x^2 over up to 2^18 rows are exact in f32"""
    s = 100 * seed + rows + C
    rs = storage_rounding(dtype)
    g = torch.Generator().manual_seed(s)
    if exact:
        x, dy, res = (dyadic(rows, C, seed=s + n, lo=-8, hi=8, denom=8) for n in (1, 2, 3))
    else:
        sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
        x = rs(std * (torch.randn(rows, C, generator=g) + ratio * sign))
        dy, res = rs(torch.randn(rows, C, generator=g)), rs(std * torch.randn(rows, C, generator=g))
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(C, generator=g)
    return dict(x=x, dy=dy, res=res, gamma=u(0.5, 1.5) * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1), beta=std * u(-1, 1),
                rmean=std * u(-1, 1), rvar=std * std * u(0.5, 1.5))


DCN_BORDER_CLASSES = ('integer', 'above_top', 'below_bottom', 'far_before', 'far_after', 'mixed')


def dcn_inputs(dtype, B, H, W, C, kind='random', seed=0, logit_scale=1.0):
    """-> dict x [M, C], dcol [M, 9 * C] (rounded to dtype), om [M, 32] f32 (columns 27..31 hold NaN: never read).
    kind 'random': offsets N(0, 1.5) (many samples leave a small image), or one border class for EVERY tap of every pixel:
      'integer'      offsets in {-1, 0, 1}: the sample sits on a pixel, wy = wx = 0, the +1 corners weigh nothing
      'above_top'    py in (-1, 0): the y0 = -1 corners are invalid, the y0 + 1 = 0 ones valid; same in x
      'below_bottom' py in (H - 1, H): the y0 + 1 = H corners are invalid
      'far_before'   py <= -1 and px < -1: no corner contributes (py = -1 exactly is among them: the y0 + 1 = 0 corners are then
                     valid in y with weight 0, and px keeps all four outside);  'far_after'  py >= H and px > W: likewise
      'mixed'        the classes above cycled over the taps of a pixel
      'dyadic'       offsets drawn from {0, +-1, +-0.5}: bilinear weights in {0, 1/4, 1/2, 1}, logits 0 (m = 1/2 exactly)"""
    M = B * H * W
    g = torch.Generator().manual_seed(50 * seed + M + C)
    rs = storage_rounding(dtype)
    p = torch.arange(M)
    yy, xx = ((p // W) % H).float()[:, None], (p % W).float()[:, None]
    ky, kx = (torch.arange(9) // 3 - 1).float()[None], (torch.arange(9) % 3 - 1).float()[None]
    frac = 0.125 + 0.75 * torch.rand(M, 9, 2, generator=g)

    def target(cls):                                                       # sample points [M, 9] in y and x
        if cls == 'integer':
            d = torch.randint(-1, 2, (M, 9, 2), generator=g).float()
            return yy + ky + d[..., 0], xx + kx + d[..., 1]
        if cls == 'above_top':
            return -frac[..., 0], -frac[..., 1]
        if cls == 'below_bottom':
            return H - 1 + frac[..., 0], W - 1 + frac[..., 1]
        if cls == 'far_before':
            return -1 - 2 * frac[..., 0] * (frac[..., 1] > 0.5), -1 - 3 * frac[..., 1]
        return H + 2 * frac[..., 0] * (frac[..., 1] > 0.5), W + 3 * frac[..., 1]
    om = torch.full((M, 32), float('nan'))
    om[:, 18:27] = logit_scale * torch.randn(M, 9, generator=g)
    if logit_scale >= 30:                                                  # exactly +-logit_scale: the sigmoid saturates, exp stays finite
        om[:, 18:27] = logit_scale * torch.sign(om[:, 18:27])
    if kind == 'random':
        om[:, :18] = 1.5 * torch.randn(M, 18, generator=g)
    elif kind == 'dyadic':
        om[:, :18] = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5])[torch.randint(0, 5, (M, 18), generator=g)]
        om[:, 18:27] = 0.0
    else:
        classes = DCN_BORDER_CLASSES[:5]
        ty, tx = torch.zeros(M, 9), torch.zeros(M, 9)
        for i, cls in enumerate(classes):
            cy, cx = target(cls)
            sel = torch.full((9,), kind == cls) if kind != 'mixed' else (torch.arange(9) % 5 == i)
            ty, tx = torch.where(sel[None], cy + 0 * ty, ty), torch.where(sel[None], cx + 0 * tx, tx)
        om[:, 0:18:2], om[:, 1:18:2] = ty - (yy + ky), tx - (xx + kx)
    if kind == 'dyadic':
        x, dcol = dyadic(M, C, seed=seed + 1, lo=-8, hi=8, denom=8), dyadic(M, 9 * C, seed=seed + 2, lo=-4, hi=4, denom=4)
    else:
        x, dcol = rs(signed_magnitudes(M, C, seed=seed + 1)), rs(signed_magnitudes(M, 9 * C, seed=seed + 2))
    return dict(x=x, dcol=dcol, om=om)


# ------------------------------------------------------------------------------------------------ LeFF depthwise 3x3 (csrc/fw_elem.hip)
# fw_dwconv_fwd / fw_dwconv_bwd: the plain f64 statement, element-wise bounds counted from the kernels' roundings, and a restatement
# of the host dispatch (which of the five kernels a call reaches, and with which walk).  Tensors are [B*H*W, >= C] float64 holding
# storage-rounded values, on the host or the device; w is [C, 9] in the parameter's own layout (the ABI takes its transpose), bias [C].
#   fwd : h2 = bias + sum_(ky,kx) w[ky,kx] g[y + ky - 1][x + kx - 1],  g = GELU(h1) (in_gelu) or the stored g1;  g2 = GELU(h2)
#   bwd : dh1 = GELU'(h1) sum_(ky,kx) w[ky,kx] dh2[y - ky + 1][x - kx + 1]
#         dw[c][ky,kx] += sum_p g[p] dh2[p - (ky,kx) + 1],  dbias[c] += sum_p dh2[p]
# The constants below restate csrc/fw_elem.hip; tests/test_dwconv_bounds_cpu.py reads them back out of the source.
DW_TILED_MIN = 10_000_000         # B*H*W*C from which the LDS-tiled forms run (H % DT_TY == 0 as well)
DT_TY, DT_TX, DT_CB = 8, 16, 64   # a tile: rows x pixels x channels
DW_SX = 8                         # SX: pixels of a strip
WG_VL, WG_SL = 32, 8              # weight-gradient block: channel vectors x strip lanes
DW_FWD_WANT, DW_BWD_WANT = 2048, 1024   # workgroups the pipelined forward / the fused backward aim for
DW_NT_MAX = 32                    # tile rows a workgroup walks at most
DW_NSTRIP_MAX, DW_WG_MIN_BLOCKS = 16, 384
DW_STRIP_GRID_CAP = 8192          # grid_for: workgroups of 256 threads, then a grid-stride loop
DW_TPB = 256
DW_TAP_ROUNDINGS = 9 + 1 + 1      # nine taps, the bias (forward) or the product with GELU' (backward), one spare
DW_MUTATIONS = ('halo_top_neighbour', 'halo_bottom_neighbour', 'col_left_clamped', 'col_right_clamped', 'taps_not_flipped',
                'kykx_swapped', 'cblock_dropped', 'half_tile_dropped', 'beyond_w_counted', 'gelu_missing', 'gelu_twice',
                'gelu_grad_at_gelu', 'dw_tap_reversed', 'prefill_overwritten', 'tile_row_dropped')


def _cdiv(a, b):
    return -(-a // b)


def _dw_walk(B, H, W, C, want):
    """the persistent tile walk of dwconv_fwd_pipe_kernel / dwconv_bwd_fused_kernel: ncol tile columns (channel block x 16 pixels),
    nrow = B * H / 8 tile rows numbered straight through the images, NT consecutive rows per workgroup"""
    ntx, nty = _cdiv(W, DT_TX), H // DT_TY
    ncol, nrow = _cdiv(C, DT_CB) * ntx, B * nty
    raw = ncol * nrow // want
    NT = min(max(raw, 1), DW_NT_MAX)
    nchunk = _cdiv(nrow, NT)
    wgs = ncol * nchunk
    return dict(NT=NT, raw=raw, ncol=ncol, ntx=ntx, nrow=nrow, nchunk=nchunk, wgs=wgs, wgs_padded=rup(wgs, 8), idle=rup(wgs, 8) - wgs,
                crossing=sum(1 for r in range(nty, nrow, nty) if r % NT), last_walk=nrow - (nchunk - 1) * NT)


def dwconv_plan(B, H, W, C, ld, dtype, g1):
    """What fw_dwconv_fwd (input row stride ld) and fw_dwconv_bwd (dh2 / h1 row stride ld, g1 kept or not) launch for this shape.
    -> dict fwd / bwd: 'form' and the launch arithmetic of that form.
      fwd form 'strip' | 'fwd_pipe' | 'tile';  bwd form 'strip+wgrad' | 'fused' | 'tile+wgrad'
      walks (fwd_pipe, fused): NT, raw (the quotient before the clamp), nchunk (walks per tile column), wgs / wgs_padded / idle
        (workgroups before and after padding to 8, and the padded ones that find no walk), crossing (walks of a column that cross an
        image border), last_walk (tile rows of the last walk)
      strip: grid (padded to 8), threads, passes of the grid-stride loop;  tile: wgs, wgs_padded
      bwd also: NSTRIP, wgrad_blocks, nsg (weight-gradient blocks per channel group) whether or not the weight-gradient kernel runs,
      and dw_depth: the longest chain of f32 additions between one product and dw / dbias in the form that runs."""
    assert dtype in (torch.float32, torch.bfloat16)
    tiled = H % DT_TY == 0 and B * H * W * C >= DW_TILED_MIN
    off32 = H * W * ld < 2 ** 31
    n = B * H * (W // DW_SX) * (C // 4)
    grid = rup(min(max(_cdiv(n, DW_TPB), 1), DW_STRIP_GRID_CAP), 8)
    strip = dict(grid=grid, threads=n, passes=_cdiv(n, grid * DW_TPB))
    nb = B * (H // DT_TY) * _cdiv(W, DT_TX) * _cdiv(C, DT_CB)
    tile = dict(wgs=nb, wgs_padded=rup(nb, 8))
    if tiled and off32:
        fwd = dict(form='fwd_pipe', **_dw_walk(B, H, W, C, DW_FWD_WANT))
    elif tiled:
        fwd = dict(form='tile', **tile)
    else:
        fwd = dict(form='strip', **strip)
    nvg, nst = _cdiv(C // 4, WG_VL), B * H * (W // DW_SX)
    NSTRIP = DW_NSTRIP_MAX
    while NSTRIP > 2 and _cdiv(nst, NSTRIP * WG_SL) * nvg < DW_WG_MIN_BLOCKS:
        NSTRIP >>= 1
    nsg = _cdiv(nst, NSTRIP * WG_SL)
    wg = dict(NSTRIP=NSTRIP, nsg=nsg, wgrad_blocks=nsg * nvg, dead_lanes=C // 4 % WG_VL != 0)
    # chains: a product (one rounding in f32), then
    #   wgrad: 8 pixels x NSTRIP strips into a register, one shuffle, the four waves' LDS atomics, one global atomic per block of the
    #          channel group;   fused: 8 pixels into gk, NT tiles into the LDS partial (dbias: 8 x NT into a register), two shuffles,
    #          the four waves, one global atomic per workgroup of the same channel block (ntx * nchunk of them)
    if tiled and not g1 and off32:
        walk = _dw_walk(B, H, W, C, DW_BWD_WANT)
        bwd = dict(form='fused', **walk, **wg, dw_depth=1 + 8 * walk['NT'] + walk['NT'] + 2 + 4 + walk['ntx'] * walk['nchunk'])
    else:
        bwd = dict(form='tile+wgrad' if tiled else 'strip+wgrad', **(tile if tiled else strip), **wg, dw_depth=1 + 8 * NSTRIP + 1 + 4 + nsg)
    return dict(fwd=fwd, bwd=bwd)


def _dw_add_tap(acc, x4, wk, dy, dx, flat_rows=False, clamp=None):
    """acc[b, y, x] += wk * x4[b, y + dy, x + dx], zero outside the image.  flat_rows: the rows of all images taken as one tall image
    (a halo row then comes from the neighbouring image); clamp 'left' / 'right': the column outside the image reads the edge column"""
    if flat_rows:
        acc, x4 = acc.view(1, -1, *acc.shape[2:]), x4.view(1, -1, *x4.shape[2:])
    H, W = acc.shape[1:3]
    ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    acc[:, ya:yb, xa:xb].addcmul_(x4[:, ya + dy:yb + dy, xa + dx:xb + dx], wk)
    if clamp == 'left' and dx == -1:
        acc[:, ya:yb, 0].addcmul_(x4[:, ya + dy:yb + dy, 0], wk)
    if clamp == 'right' and dx == 1:
        acc[:, ya:yb, W - 1].addcmul_(x4[:, ya + dy:yb + dy, W - 1], wk)


def _dw_stencil(x4, w9, flip, mutation=None):
    """sum over the nine taps of w[c][ky,kx] x4[y + s (ky - 1)][x + s (kx - 1)], s = +1 (forward) or -1 (flip: the data gradient)"""
    acc = torch.zeros_like(x4)
    s = -1 if flip and mutation != 'taps_not_flipped' else 1
    for ky in range(3):
        for kx in range(3):
            k = kx * 3 + ky if mutation == 'kykx_swapped' else ky * 3 + kx
            dy, dx = s * (ky - 1), s * (kx - 1)
            flat = (mutation == 'halo_top_neighbour' and dy == -1) or (mutation == 'halo_bottom_neighbour' and dy == 1)
            clamp = {'col_left_clamped': 'left', 'col_right_clamped': 'right'}.get(mutation)
            _dw_add_tap(acc, x4, w9[:, k], dy, dx, flat, clamp)
    return acc


def _dw_unwritten(v4, C, W, mutation):
    """what a kernel that skips its last partial channel block, or its half-width last tile column, leaves of an output: nothing"""
    if mutation == 'cblock_dropped' and C % DT_CB:
        v4[..., C // DT_CB * DT_CB:] = 0
    if mutation == 'half_tile_dropped' and W % DT_TX == 8:
        v4[:, :, W - 8:] = 0
    return v4


def dw_touched(mutation, B, H, W, C):
    """[B, H, W, C] mask of the data-output elements (h2, g2, dh1) a mutation of the stencil changes"""
    m = torch.zeros(B, H, W, C, dtype=torch.bool)
    if mutation == 'halo_top_neighbour':
        m[1:, 0] = True
    elif mutation == 'halo_bottom_neighbour':
        m[:-1, H - 1] = True
    elif mutation == 'col_left_clamped':
        m[:, :, 0] = True
    elif mutation == 'col_right_clamped':
        m[:, :, W - 1] = True
    elif mutation == 'cblock_dropped':
        m[..., C // DT_CB * DT_CB:] = C % DT_CB != 0
    elif mutation == 'half_tile_dropped':
        m[:, :, W - 8:] = W % DT_TX == 8
    else:
        m[:] = True
    return m.reshape(B * H * W, C)


def dwconv_ref(src, in_gelu, w, bias, B, H, W, C, dtype, mutation=None):
    """fw_dwconv_fwd in f64.  src [B*H*W, >= C]: the pre-activation h1 (in_gelu) or the stored activation g1.
    -> {'h2': (value, tol), 'g2': (value, tol)}, each [B*H*W, C].
    h2: DW_TAP_ROUNDINGS f32 roundings of partial sums that |bias| + sum |w| |g| bounds, plus sum |w| (operand error of g), plus the
    storage rounding.  With in_gelu the operand error is gelu_operand_err: GELU's own value error AND, in bf16, the re-rounding of
    GELU(h1) to bf16 on its way into LDS.  Only dwconv_tile_kernel and dwconv_fwd_pipe_kernel re-round; dwconv_strip_kernel (and
    both weight-gradient forms and the fused backward) keep GELU(h1) in f32 -- the bound is stated once, for the larger variant.
    g2 = GELU of the f32 sum (not of the stored h2): the `twin` branch of gemm_expect."""
    x4 = src[:, :C].reshape(B, H, W, C).contiguous()
    err4 = None
    if in_gelu:
        err4 = gelu_operand_err(x4, dtype)
        if mutation != 'gelu_missing':
            x4 = gelu64(gelu64(x4)) if mutation == 'gelu_twice' else gelu64(x4)
    v = _dw_stencil(x4, w, False, mutation) + bias
    mag = _dw_stencil(x4.abs(), w.abs(), False) + bias.abs()
    tol = DW_TAP_ROUNDINGS * U32 * mag
    if err4 is not None:
        tol = tol + _dw_stencil(err4, w.abs(), False)
    v = _dw_unwritten(v, C, W, mutation)
    t_val = gelu64(v)
    t_tol = GELU_LIPSCHITZ * tol + gelu_value_err(v.abs() + tol, dtype)
    if dtype == torch.bfloat16:
        tol, t_tol = tol + UBF * (v.abs() + tol), t_tol + UBF * (t_val.abs() + t_tol)
    f = lambda t: t.reshape(B * H * W, C)
    return dict(h2=(f(v), f(tol)), g2=(f(t_val), f(t_tol)))


def dwconv_bwd_ref(dh2, g1, h1, w, B, H, W, C, dtype, ld=None, dw0=None, db0=None, mutation=None, drop=None):
    """fw_dwconv_bwd in f64.  dh2, h1 (and g1, or None: the kernels evaluate GELU(h1)) [B*H*W, >= C]; dw0 [C, 9] / db0 [C]: what dw /
    dbias hold before the call (the kernels ADD to them).  ld: the row stride of dh2 / h1 the dispatch sees (default C).
    drop = (b, y0, y1): the INPUT pixels of rows [y0, y1) of image b left out of dw / dbias (a tile row a walk skipped).
    -> {'dh1': (value, tol) [B*H*W, C], 'dw': (value, tol) [C, 9], 'dbias': (value, tol) [C]}.
    dh1: the flipped-tap sum s with DW_TAP_ROUNDINGS roundings, times GELU'(h1): tol_s (|GELU'| + e') + |s| e' + storage.
    dw / dbias: depth u (sum |g| |dh2| + |prefill|) for ANY order of the additions, depth = the longest chain of the form that
    dwconv_plan names (zero terms add nothing to the magnitude sum), plus sum |dh2| (GELU value error) where GELU is evaluated
    in-kernel (kept in f32 there: no re-rounding)."""
    d4 = dh2[:, :C].reshape(B, H, W, C).contiguous()
    h4 = h1[:, :C].reshape(B, H, W, C).contiguous()
    s = _dw_stencil(d4, w, True, mutation)
    tol_s = DW_TAP_ROUNDINGS * U32 * _dw_stencil(d4.abs(), w.abs(), True)
    gp = gelu_grad64(gelu64(h4) if mutation == 'gelu_grad_at_gelu' else h4)
    eg = gelu_grad_value_err(dtype)
    v = _dw_unwritten(s * gp, C, W, mutation)
    tol = tol_s * (gp.abs() + eg) + s.abs() * eg
    if dtype == torch.bfloat16:
        tol = tol + UBF * (v.abs() + tol)
    # ---- weight / bias gradient
    if g1 is not None:
        g4, ge4 = g1[:, :C].reshape(B, H, W, C).contiguous(), None
        if mutation == 'gelu_twice':
            g4 = gelu64(g4)
    else:
        ge4 = gelu_value_err(h4, dtype)
        g4 = h4 if mutation == 'gelu_missing' else (gelu64(gelu64(h4)) if mutation == 'gelu_twice' else gelu64(h4))
    db4 = d4
    if drop is not None or mutation == 'half_tile_dropped':
        g4, db4 = g4.clone(), d4.clone()
        if drop is not None:
            b, y0, y1 = drop
            g4[b, y0:y1] = 0
            db4[b, y0:y1] = 0
        if mutation == 'half_tile_dropped' and W % DT_TX == 8:
            g4[:, :, W - 8:] = 0
            db4[:, :, W - 8:] = 0
    dw, mag, gerr = (torch.zeros(C, 9, dtype=d4.dtype, device=d4.device) for _ in range(3))
    for ky in range(3):
        for kx in range(3):
            dy, dx = 1 - ky, 1 - kx                                        # dh2 at p + (dy, dx) meets the input pixel p
            flat = (mutation == 'halo_top_neighbour' and dy == -1) or (mutation == 'halo_bottom_neighbour' and dy == 1)
            a, b_ = (g4.view(1, B * H, W, C), d4.view(1, B * H, W, C)) if flat else (g4, d4)
            Hh = a.shape[1]
            ya, yb, xa, xb = max(0, -dy), min(Hh, Hh - dy), max(0, -dx), min(W, W - dx)
            gs, ds = a[:, ya:yb, xa:xb], b_[:, ya + dy:yb + dy, xa + dx:xb + dx]
            k = ky * 3 + kx
            dw[:, k] = torch.einsum('byxc,byxc->c', gs, ds)
            mag[:, k] = torch.einsum('byxc,byxc->c', gs.abs(), ds.abs())
            if ge4 is not None:
                gerr[:, k] = torch.einsum('byxc,byxc->c', ge4[:, ya:yb, xa:xb], d4[:, ya + dy:yb + dy, xa + dx:xb + dx].abs())
            if (mutation == 'col_left_clamped' and dx == -1) or (mutation == 'col_right_clamped' and dx == 1):
                col = 0 if dx == -1 else W - 1                             # the column outside the image reads the edge column
                dw[:, k] += torch.einsum('byc,byc->c', g4[:, ya:yb, col], d4[:, ya + dy:yb + dy, col])
            if mutation == 'beyond_w_counted' and kx == 2 and W % DT_TX == 8:
                # the clamped strip beyond W holds g[W - 1] again; its first pixel (x = W) meets dh2[W - 1] at kx = 2
                dw[:, k] += torch.einsum('byc,byc->c', g4[:, ya:yb, W - 1], d4[:, ya + dy:yb + dy, W - 1])
    db = db4.sum((0, 1, 2))
    dbmag = db4.abs().sum((0, 1, 2))
    if mutation == 'beyond_w_counted' and W % DT_TX == 8:
        db = db + 8 * d4[:, :, W - 1].sum((0, 1))                          # eight clamped columns counted as pixels
    if mutation == 'cblock_dropped' and C % DT_CB:
        dw[C // DT_CB * DT_CB:] = 0
        db[C // DT_CB * DT_CB:] = 0
    if mutation == 'dw_tap_reversed':
        dw = dw.flip(1)
    dw0 = torch.zeros_like(dw) if dw0 is None else dw0.to(dw)
    db0 = torch.zeros_like(db) if db0 is None else db0.to(db)
    if mutation != 'prefill_overwritten':
        dw, db = dw + dw0, db + db0
    depth = dwconv_plan(B, H, W, C, ld or C, dtype, g1 is not None)['bwd']['dw_depth']
    tol_w = depth * U32 * (mag + dw0.abs()) + gerr
    tol_b = depth * U32 * (dbmag + db0.abs())
    return dict(dh1=(v.reshape(B * H * W, C), tol.reshape(B * H * W, C)), dw=(dw, tol_w), dbias=(db, tol_b))


def dwconv_rows_share(dh2, g, B, H, W, C, b, y0, y1):
    """what the INPUT pixels of rows [y0, y1) of image b add to dw and dbias (g: the activation the weight gradient multiplies, f64):
    the weight-gradient statement on the window of rows that those pixels' taps reach.  -> (dw part [C, 9], dbias part [C])"""
    ya, yb = max(0, y0 - 1), min(H, y1 + 1)
    d4 = dh2[:, :C].reshape(B, H, W, C)[b:b + 1, ya:yb]
    gm = torch.zeros_like(d4)
    gm[0, y0 - ya:y1 - ya] = g[:, :C].reshape(B, H, W, C)[b, y0:y1]
    part = dwconv_bwd_ref(d4.reshape(-1, C), gm.reshape(-1, C), gm.reshape(-1, C), torch.zeros(C, 9, dtype=d4.dtype, device=d4.device),
                          1, yb - ya, W, C, torch.float32)
    return part['dw'][0], d4[0, y0 - ya:y1 - ya].sum((0, 1))
