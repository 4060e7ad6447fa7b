"""Structural-similarity loss on the device (fw_ssim11_loss, csrc/fw_loss.hip): the reference's utils/pytorch_ssim/__init__.py:19-43
(Gaussian 11x11 window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over the map), value and gradient in one launch.

    SSIMLossFn.apply(restored, clean, gscale) -> f32 [1] = SSIM; d/d restored is the kernel's gradient times gscale
    ssim11(a, b)                              -> the value alone, for [C, H, W] or [B, C, H, W] images, f32 or u8

The training step adds the term inside the L1 loss's launch sequence instead (engine.TrainLossFn / L1LossFn with `ssim`): the kernel
then accumulates into the gradient buffer fw_l1_loss filled.  The evaluation metric of results.log is another SSIM (fw_ssim7: skimage's
7x7 uniform window, evaluate.ssim)."""
import torch

from .lib import call


def _planes(x):
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4:
        raise ValueError(f'fwair.losses: expected [C, H, W] or [B, C, H, W], got {tuple(x.shape)}')
    if x.dtype == torch.uint8:
        x = x.float().div_(255.0)
    elif x.dtype != torch.float32:
        raise TypeError(f'fwair.losses: f32 or u8 images, got {x.dtype}')
    return x.contiguous()


def ssim11_launch(restored, clean, dres, gscale, accumulate, out):
    """out[0] += SSIM(restored, clean); dres (+)= gscale * dSSIM/d restored (dres may be None).  f32 [B, C, H, W] contiguous."""
    B, C, H, W = restored.shape
    if restored.shape != clean.shape:
        raise ValueError(f'fwair.losses: shapes differ: {tuple(restored.shape)} vs {tuple(clean.shape)}')
    call('fw_ssim11_loss', restored, clean, dres, B, C, H, W, float(gscale), 1 if accumulate else 0, out)


class SSIMLossFn(torch.autograd.Function):
    """mean SSIM(restored, clean) (f32 [1]); the gradient is pre-scaled by gscale, as engine.L1LossFn's is."""

    @staticmethod
    def forward(ctx, restored, clean, gscale):
        ctx.shape = restored.shape
        restored, clean = _planes(restored), _planes(clean)
        out = torch.zeros(1, dtype=torch.float32, device=restored.device)
        dres = torch.empty_like(restored)
        ssim11_launch(restored, clean, dres, gscale, False, out)
        ctx.save_for_backward(dres)
        return out

    @staticmethod
    def backward(ctx, dout):
        return ctx.saved_tensors[0].view(ctx.shape), None, None


def ssim11(a, b):
    """SSIM of two images or batches on the device, value only -> 0-dim f32 tensor.  u8 inputs are divided by 255."""
    a, b = _planes(a), _planes(b)
    out = torch.zeros(1, dtype=torch.float32, device=a.device)
    ssim11_launch(a, b, None, 0.0, False, out)
    return out[0]
