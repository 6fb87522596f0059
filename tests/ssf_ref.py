"""Plain-torch restatement of the scale-space-flow video model (``ssf2020``: Agustsson et al., CVPR 2020, as CompressAI publishes it)
and of its two operators, the scale-space volume and the trilinear warp through it.  The reference of tests/test_ssf_cpu.py
(state_dict keys and shapes, the two identities that pin the operators' definition) and, run in float64, of
tests/test_ssf_kernels_gpu.py and tests/test_ssf_model_gpu.py.

volume: nn.functional.conv2d with the outer product of the Gaussian taps on a replicate-padded frame, avg_pool2d, F.interpolate.
warp: F.grid_sample(volume, identity grid + (flow | scale), padding_mode="border", align_corners=False).
model: nn.Conv2d / nn.ConvTranspose2d / nn.ReLU plus the oracle's EntropyBottleneck and GaussianConditional.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.leaves import CompressionModel, EntropyBottleneck, GaussianConditional  # noqa: F401


# ------------------------------------------------------------------------------------------------------------------ operators
def gaussian_kernel1d(sigma0, dtype=torch.float64, device=None):
    k = 2 * int(math.ceil(3 * sigma0)) + 1
    t = torch.linspace(-(k - 1) / 2, (k - 1) / 2, k, dtype=dtype, device=device)
    g = torch.exp(-0.5 * (t / sigma0) ** 2)
    return g / g.sum()


def blur(x, g):
    k, Cc = g.numel(), x.shape[1]
    xp = F.pad(x, (k // 2,) * 4, mode="replicate")
    return F.conv2d(xp, torch.outer(g, g).to(x.dtype)[None, None].expand(Cc, 1, k, k), groups=Cc)


def volume(x, sigma0=1.5, num_levels=5):
    """x [N, C, H, W] -> [N, C, num_levels + 1, H, W]"""
    g = gaussian_kernel1d(sigma0, x.dtype, x.device)
    slices = [x]
    t = blur(x, g)
    slices.append(t)
    for i in range(1, num_levels):
        t = blur(F.avg_pool2d(t, kernel_size=(2, 2), stride=(2, 2)), g)
        up = t
        for _ in range(i):
            up = F.interpolate(up, scale_factor=2, mode="bilinear", align_corners=False)
        slices.append(up)
    return torch.stack(slices, dim=2)


def warp_grid(flow, scale):
    """the sampling grid [N, 1, H, W, 3] in normalised (x, y, z) coordinates"""
    N, _, H, W = flow.shape
    gx = ((2 * torch.arange(W, dtype=flow.dtype, device=flow.device) + 1) / W - 1).view(1, 1, W).expand(N, H, W)
    gy = ((2 * torch.arange(H, dtype=flow.dtype, device=flow.device) + 1) / H - 1).view(1, H, 1).expand(N, H, W)
    return torch.stack((gx + flow[:, 0], gy + flow[:, 1], scale[:, 0]), dim=-1).unsqueeze(1)


def warp(vol, flow, scale):
    """vol [N, C, D, H, W], flow [N, 2, H, W], scale [N, 1, H, W] -> [N, C, H, W]"""
    return F.grid_sample(vol, warp_grid(flow, scale), mode="bilinear", padding_mode="border", align_corners=False).squeeze(2)


def pixel_indices(flow, scale, D):
    """the unclamped (ix, iy, iz) of every pixel, [N, H, W] each"""
    g = warp_grid(flow, scale)[:, 0]
    N, H, W, _ = g.shape
    return ((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2, ((g[..., 2] + 1) * D - 1) / 2


# ---------------------------------------------------------------------------------------------------------------------- model
def conv(i, o, kernel_size=5, stride=2):
    return nn.Conv2d(i, o, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2)


def deconv(i, o, kernel_size=5, stride=2):
    return nn.ConvTranspose2d(i, o, kernel_size=kernel_size, stride=stride, output_padding=stride - 1, padding=kernel_size // 2)


class _QReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bit_depth, beta):
        ctx.alpha, ctx.beta, ctx.max_value = 0.9943258522851727, beta, 2 ** bit_depth - 1
        ctx.save_for_backward(x)
        return x.clamp(min=0, max=ctx.max_value)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        sub = torch.exp(-ctx.alpha ** ctx.beta * torch.abs(2.0 * x / ctx.max_value - 1) ** ctx.beta) * g
        out = g.clone()
        out[x < 0] = sub[x < 0]
        out[x > ctx.max_value] = sub[x > ctx.max_value]
        return out, None, None


def qrelu(x, bit_depth=8, beta=100):
    return _QReLUFn.apply(x, bit_depth, beta)


class Encoder(nn.Sequential):
    def __init__(self, in_planes, mid_planes=128, out_planes=192):
        super().__init__(conv(in_planes, mid_planes), nn.ReLU(inplace=True), conv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         conv(mid_planes, mid_planes), nn.ReLU(inplace=True), conv(mid_planes, out_planes))


class Decoder(nn.Sequential):
    def __init__(self, out_planes, in_planes=192, mid_planes=128):
        super().__init__(deconv(in_planes, mid_planes), nn.ReLU(inplace=True), deconv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         deconv(mid_planes, mid_planes), nn.ReLU(inplace=True), deconv(mid_planes, out_planes))


class HyperEncoder(nn.Sequential):
    def __init__(self, in_planes=192, mid_planes=192, out_planes=192):
        super().__init__(conv(in_planes, mid_planes), nn.ReLU(inplace=True), conv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         conv(mid_planes, out_planes))


class HyperDecoder(nn.Sequential):
    def __init__(self, in_planes=192, mid_planes=192, out_planes=192):
        super().__init__(deconv(in_planes, mid_planes), nn.ReLU(inplace=True), deconv(mid_planes, mid_planes), nn.ReLU(inplace=True),
                         deconv(mid_planes, out_planes))


class HyperDecoderWithQReLU(nn.Module):
    def __init__(self, in_planes=192, mid_planes=192, out_planes=192):
        super().__init__()
        self.deconv1 = deconv(in_planes, mid_planes)
        self.deconv2 = deconv(mid_planes, mid_planes)
        self.deconv3 = deconv(mid_planes, out_planes)

    def forward(self, x):
        return qrelu(self.deconv3(qrelu(self.deconv2(qrelu(self.deconv1(x))))))


class Hyperprior(CompressionModel):
    def __init__(self, planes=192, mid_planes=192):
        super().__init__(entropy_bottleneck_channels=mid_planes)
        self.hyper_encoder = HyperEncoder(planes, mid_planes, planes)
        self.hyper_decoder_mean = HyperDecoder(planes, mid_planes, planes)
        self.hyper_decoder_scale = HyperDecoderWithQReLU(planes, mid_planes, planes)
        self.gaussian_conditional = GaussianConditional(None)

    def forward(self, y):
        z = self.hyper_encoder(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales = self.hyper_decoder_scale(z_hat)
        means = self.hyper_decoder_mean(z_hat)
        _, y_likelihoods = self.gaussian_conditional(y, scales, means)
        y_hat = (torch.round(y - means) - (y - means)).detach() + (y - means) + means   # quantize_ste(y - means) + means
        return y_hat, {"y": y_likelihoods, "z": z_likelihoods}, (y - means)


class ScaleSpaceFlow(CompressionModel):
    """The hyperpriors are Hyperprior(planes, planes): CompressAI builds them with its defaults (192, 192), which are `planes` at the
    default width; mid_planes sizes the six encoders / decoders only."""

    def __init__(self, num_levels=5, sigma0=1.5, scale_field_shift=1.0, mid_planes=128, planes=192):
        super().__init__()
        self.img_encoder = Encoder(3, mid_planes, planes)
        self.img_decoder = Decoder(3, planes, mid_planes)
        self.img_hyperprior = Hyperprior(planes, planes)
        self.res_encoder = Encoder(3, mid_planes, planes)
        self.res_decoder = Decoder(3, 2 * planes, mid_planes)
        self.res_hyperprior = Hyperprior(planes, planes)
        self.motion_encoder = Encoder(2 * 3, mid_planes, planes)
        self.motion_decoder = Decoder(2 + 1, planes, mid_planes)
        self.motion_hyperprior = Hyperprior(planes, planes)
        self.sigma0, self.num_levels, self.scale_field_shift = sigma0, num_levels, scale_field_shift
        self.residuals = []   # every (y - means) of the last forward: the test checks their distance from the rounding points

    def forward(self, frames):
        self.residuals = []
        x_hat, lik = self.forward_keyframe(frames[0])
        recs, liks = [x_hat], [lik]
        x_ref = x_hat.detach()
        for x in frames[1:]:
            x_ref, lik = self.forward_inter(x, x_ref)
            recs.append(x_ref)
            liks.append(lik)
        return {"x_hat": recs, "likelihoods": liks}

    def forward_keyframe(self, x):
        y_hat, lik, r = self.img_hyperprior(self.img_encoder(x))
        self.residuals.append(r)
        return self.img_decoder(y_hat), {"keyframe": lik}

    def forward_inter(self, x_cur, x_ref):
        y_m_hat, m_lik, r = self.motion_hyperprior(self.motion_encoder(torch.cat((x_cur, x_ref), dim=1)))
        self.residuals.append(r)
        info = self.motion_decoder(y_m_hat)
        x_pred = warp(volume(x_ref, self.sigma0, self.num_levels), info[:, :2], info[:, 2:3])
        y_r_hat, r_lik, r = self.res_hyperprior(self.res_encoder(x_cur - x_pred))
        self.residuals.append(r)
        x_rec = x_pred + self.res_decoder(torch.cat((y_r_hat, y_m_hat), dim=1))
        return x_rec, {"motion": m_lik, "residual": r_lik}
