"""Power-law / band-pass spectral noise (API of the reference's ``py/nodes/powernoise.py``).

Setup (host, once per sampler): the rfft-space gain ``filter[H, W/2+1]`` is built with the reference's
exact recipe (it is *not* a closed-form 1/f: oversampled grid + bilinear resample), and the C x C
channel mixer is factorised.  Per call (device): one fused kernel draws (or replays) the complex
half-spectrum, multiplies by the filter, runs the LDS-resident C2R inverse FFT and accumulates the
normaliser's statistics (``sonar_power_irfft2_f32``); mixing and normalisation are HIP kernels too.
"""
from __future__ import annotations

import importlib
import math
import os
import random
import tempfile

import torch
from torch import Tensor

from ... import hip_lib
from ..noise import CustomNoiseItemBase
from ..noise_generation import BrownianTreeNoiseSampler, DeviceRNG, current_batch_offset
from .. import utils
from ..utils import attach_stats, pop_stats, scale_noise


def _host_module(name: str):
    """A ComfyUI host module (``folder_paths``, ``latent_preview``, ``comfy.latent_formats``) when the pack runs inside ComfyUI, None when
    the module (or a package on the way to it) does not exist.  A module that exists and fails to import raises as it does anywhere."""
    try:
        return importlib.import_module(name)
    except ModuleNotFoundError as exc:
        if exc.name is not None and (name == exc.name or name.startswith(exc.name + ".")):
            return None
        raise  # something the host module itself imports is missing: its failure, not its absence


_PREVIEW_NAMES = random.Random()  # file-name suffixes of the preview images: its own generator, the global ``random`` state is the graph's


def make_preview_result(img, result, prefix="sonar_temp"):
    """py/nodes/powernoise.py:33-53: the image saved as a temp PNG and announced to the UI next to the node's ``result``.  Inside ComfyUI
    the file goes where ``folder_paths`` says; without that module it goes into the system's temp directory."""
    name = f"{prefix}_" + "".join(_PREVIEW_NAMES.choice("abcdefghijklmnopqrstupvxyz") for _ in range(5))
    folder_paths = _host_module("folder_paths")
    if folder_paths is not None:
        folder, filename, counter, subfolder, _ = folder_paths.get_save_image_path(name, folder_paths.get_temp_directory())
    else:
        folder, filename, counter, subfolder = tempfile.gettempdir(), name, 0, ""
    filename = f"{filename}_{counter:05}_.png"
    img.save(os.path.join(folder, filename), compress_level=1)
    return {"ui": {"images": [{"filename": filename, "subfolder": subfolder, "type": "temp"}]}, "result": result}


def _preview_device() -> torch.device:
    if not torch.cuda.is_available():
        raise hip_lib.SonarHipError("filter previews are composed by a HIP kernel: no ROCm device is available")
    return torch.device("cuda", torch.cuda.current_device())


def _to_image(levels: Tensor):
    from PIL import Image

    return Image.fromarray(levels[0, 0].cpu().numpy())


def rfft2_to_fft2(x: Tensor) -> Tensor:
    """py/nodes/powernoise.py:457-468: the full spectrum's picture from a real half-spectrum ``[..., H, W/2+1]`` on the device -- rows
    fft-shifted, the mirrored half (both axes flipped, one more row of roll for an even H, column 0 dropped and the last column too when
    the half-spectrum's width is odd) on the left.  Data movement only, in the preview kernel's addressing.  Only for previews; real
    float32 tensors (the filters): a complex one would need its mirrored half conjugated."""
    if x.is_complex():
        raise hip_lib.SonarHipError("rfft2_to_fft2: real half-spectra only (the preview's filters)")
    wh = int(x.shape[-1])
    # the panel's width depends on the half-spectrum's width alone: any W with W // 2 + 1 == wh addresses the same elements
    return hip_lib.preview_panels(x.contiguous(), None, None, 2 * (wh - 1), gain=False)


class ChannelMixer:
    """py/nodes/powernoise.py:56-104: row-normalised LDL factor of the channel correlation matrix."""

    def __init__(self, channel_count, common_mode, channel_correlation):
        self.channel_count = channel_count
        self.common_mode = common_mode
        self.channel_correlation = channel_correlation
        self.mixer = self.build() if common_mode is not None else None

    def build(self) -> Tensor:
        c, cm = self.channel_count, self.common_mode
        pairs = c * (c - 1) // 2
        given = self.channel_correlation[:pairs]
        lower = torch.cat((given * cm, torch.full((pairs - given.numel(),), cm)))
        corr = torch.eye(c).index_put_(tuple(torch.tril_indices(c, c, offset=-1)), lower)
        corr += corr.tril(-1).mT
        ld = torch.linalg.ldl_factor(corr).LD
        diag = torch.diagonal_copy(ld)
        torch.diagonal(ld)[:] = 1.0
        ld *= diag.clamp_min(0).sqrt().unsqueeze(0)
        ld /= ld.norm(dim=1, keepdim=True)
        return ld

    @property
    def is_identity(self) -> bool:
        return self.mixer is None or bool(torch.equal(self.mixer.cpu(), torch.eye(self.channel_count)))

    def to(self, *args, **kwargs):
        if self.mixer is not None:
            self.mixer = self.mixer.to(*args, **kwargs)
        return self

    def apply(self, noise, shape, copy=False, partials=None):
        if self.mixer is None:
            return noise if not copy else noise.clone()
        if shape[1] != self.channel_count:
            raise ValueError("Channel count mismatch")
        return hip_lib.channel_mix(noise, self.mixer.to(noise.device, torch.float32).contiguous(), partials)

    __call__ = apply


class PowerFilter:
    """py/nodes/powernoise.py:107-266: band-pass * 1/f**alpha gain in rfft2 layout."""

    _FIELDS = ("min_freq", "max_freq", "stretch", "rotate", "pnorm", "alpha", "scale", "rel_bw", "oversample", "compose_mode")

    def __init__(self, *, min_freq=0.0, max_freq=0.7071, stretch=1.0, rotate=0.0, pnorm=2.0, alpha=0.0, scale=1.0, rel_bw=0.125,
                 oversample=4, compose_with: "PowerFilter | None" = None, compose_mode="max"):
        self.min_freq = min_freq
        self.max_freq = max(max_freq, min_freq)
        self.stretch, self.rotate, self.pnorm, self.alpha = stretch, rotate, pnorm, alpha
        self.scale, self.rel_bw, self.oversample = scale, rel_bw, oversample
        self.compose_with, self.compose_mode = compose_with, compose_mode

    def clone(self):
        args = {k: getattr(self, k) for k in self._FIELDS}
        args["compose_with"] = None if self.compose_with is None else self.compose_with.clone()
        return self.__class__(**args)

    @classmethod
    def compose(cls, a, b, compose_mode="max"):
        if a.shape != b.shape:
            raise ValueError("Filter compose size mismatch!")
        op = {"max": torch.max, "min": torch.min, "add": torch.add, "sub": torch.sub, "mul": torch.mul}.get(compose_mode, torch.max)
        return op(a, b).clamp_(min=0.0)

    @classmethod
    def normalize(cls, op, shape, mix=1.0, normalization_factor=1.0):
        """Unit-RMS gain (lerped by normalization_factor), then lerp with a flat response by ``mix``."""
        height, width = shape[-2:]
        if mix < 1.0:
            flat = torch.ones(1, 1, height, width // 2 + 1)
            if mix <= 0.0:
                return flat
        if normalization_factor != 0:
            op *= torch.lerp(torch.scalar_tensor(1.0), 1.0 / op.square().mean().sqrt(), normalization_factor)
        if mix < 1.0:
            op = torch.lerp(flat, op, mix, out=op)
        return op

    def _radial_distance(self, height, bins, oversample):
        # oversampled fftshift(rfft2freq) grid held as complex numbers purely for 2-D rotate/stretch
        cols = torch.linspace(0, 0.5, oversample * bins)
        rows = torch.linspace(-(height // 2) / height, ((height - 1) // 2) / height, oversample * height).unsqueeze(1)
        grid = torch.complex(cols, rows)
        if abs(self.rotate) >= 1e-3:
            grid *= torch.exp(1.0j * torch.deg2rad(torch.scalar_tensor(self.rotate)))
        if self.stretch > 1.0:
            grid.real *= self.stretch
        else:
            grid.imag *= 1.0 / self.stretch
        if abs(self.pnorm - 2.0) < 1e-3:
            return grid.abs()
        return torch.view_as_real(grid).abs().pow(self.pnorm).sum(-1).pow(1.0 / self.pnorm)

    def build(self, shape, override_oversample=None, composed=True):
        oversample = self.oversample if override_oversample is None else override_oversample
        height, width = shape[-2:]
        bins = width // 2 + 1
        dist = self._radial_distance(height, bins, oversample)
        gain = torch.empty_like(dist)
        ge_min, lt_max = dist >= self.min_freq, dist < self.max_freq
        inside = ge_min & lt_max
        gain[inside] = dist[inside].pow(-self.alpha)
        # Gaussian roll-off outside the band edges
        hi = ~lt_max
        gain[hi] = math.pow(self.max_freq, -self.alpha) * torch.exp(-(dist[hi] - self.max_freq).square() / (self.rel_bw * self.max_freq) ** 2)
        if self.min_freq > 0.0:
            lo = ~ge_min
            gain[lo] = math.pow(self.min_freq, -self.alpha) * torch.exp(-(dist[lo] - self.min_freq).square() / (self.rel_bw * self.min_freq) ** 2)
        gain = torch.nn.functional.interpolate(gain[None, None, ...], (height, bins), mode="bilinear", align_corners=True)
        gain = gain.roll(-(height // 2), -2)  # undo the fftshift along rows
        if self.alpha > 0:
            gain[..., 0, 0] = 0  # the DC gain would be infinite
        if self.scale != 1.0:
            gain *= self.scale
        if composed and self.compose_with is not None:
            return self.compose(gain, self.compose_with.build(shape, override_oversample=override_oversample), self.compose_mode)
        return gain

    def preview(self, size=(128, 128), mix=1.0, normalization_factor=1.0, raw=False, kernel_gain=1 / 3, filter_gain=1 / 3):
        """py/nodes/powernoise.py:268-294: the filter's spectrum and its spatial kernel side by side.  ``raw``: the two fp32 panels
        ``[1, 1, H, .]`` (views of one device tensor), else a PIL ``L`` image."""
        size = tuple(int(v) for v in size)
        filt, kernel = self._preview_planes(size, mix, normalization_factor)
        if raw:
            panels = hip_lib.preview_panels(filt, kernel, None, size[1], filter_gain=filter_gain, kernel_gain=kernel_gain)
            split = hip_lib.preview_filter_width(size[1])
            return panels[..., :split], panels[..., split:]
        return _to_image(hip_lib.preview_compose(filt, kernel, None, size[1], filter_gain=filter_gain, kernel_gain=kernel_gain))

    def _preview_planes(self, size, mix, normalization_factor):
        """(filter [1, 1, H, W/2+1], its irfft2 [1, 1, H, W], not rolled) on the device: the filter built and normalised on the host as
        for sampling, the kernel plane from the spectral kernels with a spectrum of ones."""
        h, w = size
        if not hip_lib.power_supported(h, w):
            raise _device_irfft2_fallback_error(h, w)
        device = _preview_device()
        with utils.host_setup_threads():
            filt = self.__class__.normalize(self.build(size), (1, 4, h, w), mix=mix, normalization_factor=normalization_factor)
        filt = filt.to(device, torch.float32).reshape(1, 1, h, w // 2 + 1).contiguous()
        ones = torch.ones((1, 1, h, w // 2 + 1), dtype=torch.complex64, device=device)
        return filt, hip_lib.power_irfft2(ones, filt, (1, 1, h, w))


def _device_irfft2_fallback_error(h, w):
    return hip_lib.SonarHipError(
        f"power noise: plane {h}x{w} is beyond the spectral kernels (LDS-resident FFTs, direct passes up to 2048 x 2048); "
        "there is no CPU fallback"
    )


class PowerNoiseItem(CustomNoiseItemBase):
    """py/nodes/powernoise.py:297-408."""

    stats_lookahead = True  # device-drawn, normalised calls: see hip_lib.power_noise(lookahead=...)

    def __init__(self, factor, *, channel_correlation, power_filter=None, **kwargs):
        if isinstance(channel_correlation, str):
            vals = tuple(float(v) for v in (v.strip() for v in channel_correlation.split(",")) if v)
            channel_correlation = torch.tensor(vals, device="cpu", dtype=torch.float)
        if power_filter is None:
            fargs = {k: kwargs.pop(k) for k in ("min_freq", "max_freq", "stretch", "rotate", "pnorm", "alpha") if k in kwargs}
            power_filter = PowerFilter(**fargs)
        super().__init__(factor, power_filter=power_filter, channel_correlation=channel_correlation, **kwargs)

    def make_filter(self, shape, oversample=None):
        with utils.host_setup_threads():  # a few CPU threads: see there
            return PowerFilter.normalize(self.power_filter.build(shape, override_oversample=oversample), shape, mix=self.mix,
                                         normalization_factor=getattr(self, "filter_norm_factor", 1.0))

    def make_noise_sampler_internal(self, x: Tensor, noise_sampler, filter_rfft, normalized=True):
        """``noise_sampler`` returns a complex64 half-spectrum (replay) or None (draw on device)."""
        shape = tuple(x.shape)
        h, w = shape[-2:]
        if x.ndim < 4:
            raise hip_lib.SonarHipError("power noise: [B, C, ..., H, W] latents (4 or more dimensions)")
        if not hip_lib.power_supported(h, w):
            raise _device_irfft2_fallback_error(h, w)
        device = x.device
        filt = filter_rfft.to(device, torch.float32).reshape(h, w // 2 + 1).contiguous()
        with utils.host_setup_threads():  # the 4 x 4 LDL factorisation goes through LAPACK: its thread pool too (see there)
            mixer = ChannelMixer(shape[1], self.common_mode, self.channel_correlation)
            identity = mixer.is_identity
        mixer.to(device)
        planes_per_latent = math.prod(shape[1:-2])  # 5-D (video) latents: every [H, W] slice is a plane, as in the reference's irfft2
        # a sampler's calls take consecutive stream ids: each call leaves the next one's statistics (`stats_lookahead = False` on the item
        # or the class: every call launches its own statistics pass)
        lookahead = hip_lib.PowerLookahead() if self.stats_lookahead else None

        def sampler(sigma, sigma_next):
            z = noise_sampler(sigma, sigma_next)
            partials = hip_lib.new_partials(device)
            if self.time_brownian:
                # real noise in: rfft2 -> x filter -> irfft2, forward and inverse both LDS-resident (py/nodes/powernoise.py:356-366)
                pop_stats(z)
                noise = hip_lib.spectral_filter(z.to(device).contiguous(), filt, partials if (identity and normalized) else None)
            elif z is None:
                seed, stream = DeviceRNG.take()
                offs = current_batch_offset() * planes_per_latent
                if identity and normalized:
                    # draw + filter + FFT + normalise with a single write of the tensor
                    return hip_lib.power_noise(filt, shape, seed=seed, stream_id=stream, plane_offset=offs, factor=self.factor,
                                               lookahead=lookahead)
                noise = hip_lib.power_irfft2(None, filt, shape, seed=seed, stream_id=stream, plane_offset=offs,
                                             partials=partials if (identity and normalized) else None)
            else:
                noise = hip_lib.power_irfft2(z.to(device).contiguous(), filt, shape, partials=partials if (identity and normalized) else None)
            if not identity:
                noise = mixer(noise, shape, partials=partials)
            if defer_factor:
                return noise
            # the statistics were written by the FFT kernel (identity mixer, normalising call) or by the mixer; otherwise the
            # workspace is untouched memory and must not ride along
            have_stats = (identity and normalized) or not identity
            return scale_noise(attach_stats(noise, partials if have_stats else None), self.factor, normalized=normalized)

        defer_factor = False
        if not normalized:
            def unscaled(sigma, sigma_next):  # a chain folds the factor into its accumulation kernel (CustomNoiseChain)
                nonlocal defer_factor
                defer_factor = True
                try:
                    return sampler(sigma, sigma_next), float(self.factor)
                finally:
                    defer_factor = False

            sampler.unscaled = unscaled
        if getattr(noise_sampler, "draws_on_device", False) and not self.time_brownian:
            # a device-drawn call depends on nothing but the RNG position: traced once, then one foreign call per step (hip_lib.Planned)
            planned = hip_lib.Planned(sampler, take=DeviceRNG.take, rewind=DeviceRNG.rewind,
                                      guards=(current_batch_offset, lambda: (self.factor, self.time_brownian)))
            planned.plan_static = True
            return planned
        return sampler

    def make_noise_sampler(self, x: Tensor, sigma_min, sigma_max, *, seed, cpu: bool = True, normalized=True):
        shape = x.shape
        filter_rfft = self.make_filter(shape)
        if self.time_brownian:
            # time-correlated mode (py/nodes/powernoise.py:383-393): a real Brownian-interval field -> rfft2 -> filter -> irfft2
            if sigma_min is None:
                raise ValueError("time correlated brownian mode is valid only for stochastic samplers")
            brownian = BrownianTreeNoiseSampler(x, sigma_min, sigma_max, seed=seed, cpu=cpu)
            return self.make_noise_sampler_internal(x, brownian, filter_rfft, normalized=normalized)
        if cpu:
            def draw(_s, _sn):  # py/nodes/powernoise.py:396-402
                return torch.randn((*shape[:-1], shape[-1] // 2 + 1), dtype=torch.complex64, device="cpu")
        else:
            def draw(_s, _sn):
                return None

            draw.draws_on_device = True
        return self.make_noise_sampler_internal(x, draw, filter_rfft, normalized=normalized)

    def preview(self, size=(128, 128), noise=None, kernel_gain=1 / 3, filter_gain=1 / 3):
        """py/nodes/powernoise.py:410-454: filter spectrum, spatial kernel and a sample of the filtered noise as one ``L`` image.  Without
        ``noise`` the sample is the reference's: the seed-0 complex spectrum of a private host generator (no global RNG state moves),
        uploaded once and pushed through the filter.  A ``noise`` tensor (``[1, 1, H, W]``) is filtered as it is and NOT modified -- the
        reference multiplies its spectrum in place, which is no part of the contract.  The filter panels show the filter at mix 1."""
        size = tuple(int(v) for v in size)
        h, w = size
        if not hip_lib.power_supported(h, w):
            raise _device_irfft2_fallback_error(h, w)
        device = _preview_device()
        filt = self.make_filter(size, oversample=1).to(device, torch.float32).reshape(h, w // 2 + 1).contiguous()
        if noise is None:
            spectrum = torch.randn((1, 1, h, w // 2 + 1), dtype=torch.complex64, generator=torch.Generator().manual_seed(0))
            sample = hip_lib.power_irfft2(spectrum.to(device), filt, (1, 1, h, w))
        else:
            if tuple(noise.shape[-2:]) != size or noise.numel() != h * w:
                raise ValueError(f"preview: noise {tuple(noise.shape)} is not one {h} x {w} plane")
            # a private copy: the caller's tensor keeps its values and its statistics tag
            sample = hip_lib.spectral_filter(noise.detach().to(device, torch.float32, copy=True).reshape(1, 1, h, w).contiguous(), filt)
        pfilt, kernel = self.power_filter._preview_planes(size, 1.0, getattr(self, "filter_norm_factor", 1.0))
        return _to_image(hip_lib.preview_compose(pfilt, kernel, sample, w, filter_gain=filter_gain, kernel_gain=kernel_gain))


class PowerFilterNoiseItem(PowerNoiseItem):
    """py/nodes/powernoise.py:462-504: a power filter applied to ANOTHER noise chain (node passes time_brownian=True)."""

    def __init__(self, factor, *, noise, normalize_noise, normalize_result, **kwargs):
        super().__init__(factor, noise=noise.clone(), normalize_noise=normalize_noise, normalize_result=normalize_result, **kwargs)

    def clone_key(self, k):
        if k == "noise":
            return self.noise.clone()
        return super().clone_key(k)

    def make_noise_sampler(self, x: Tensor, sigma_min, sigma_max, *, seed, cpu: bool = True, normalized=True):
        normalize_noise = self.get_normalize("normalize_noise", False)
        normalize_result = self.get_normalize("normalize_result", normalized)
        filter_rfft = self.make_filter(x.shape)
        noise_sampler = self.noise.make_noise_sampler(x, sigma_min, sigma_max, seed, cpu, normalized=normalize_noise)
        return self.make_noise_sampler_internal(x, noise_sampler, filter_rfft, normalized=normalize_result)

    def preview(self, size=(128, 128)):
        """py/nodes/powernoise.py:524-554.  ``preview_type == "custom"``: the inner chain sampled once (seed-0 ``[1, 4, H, W]`` latent,
        sigmas 14 -> 10), filtered, decoded by ComfyUI's latent previewer and pasted over the third panel in colour.  That needs ComfyUI's
        ``latent_preview``; the reference's seed 0 is given to the host generator and to the current device's default generator (the one DeviceRNG
        hands stream ids out of) inside a fork of both: they are left as they were found, and no other generator is touched."""
        if getattr(self, "preview_type", None) != "custom":
            return super().preview(size=size)
        latent_preview = _host_module("latent_preview")
        if latent_preview is None:
            raise NotImplementedError('preview "custom" decodes the noise with ComfyUI\'s latent_preview module, which cannot be imported here')
        formats = _host_module("comfy.latent_formats")
        size = tuple(int(v) for v in size)
        device = _preview_device()
        # the reference's torch.manual_seed(0), confined: the host generator and the current device's default generator (the one DeviceRNG
        # hands stream ids out of) are seeded inside a fork of both; torch.manual_seed itself would reseed every device and stay
        with torch.random.fork_rng(devices=[device.index]):
            torch.default_generator.manual_seed(0)
            torch.cuda.manual_seed(0)
            x = torch.randn((1, 4, *size), dtype=torch.float, device="cpu").to(device)
            ns = self.noise.make_noise_sampler(x, torch.scalar_tensor(0.0), torch.scalar_tensor(14.0), 0, True,
                                               normalized=self.normalize_noise is True)
            filtered_ns = self.make_noise_sampler_internal(x, ns, self.make_filter(x.shape), self.normalize_result in {True, None})
            filtered_noise = filtered_ns(torch.scalar_tensor(14.0), torch.scalar_tensor(10.0))
        previewer = latent_preview.get_previewer(None, None if formats is None else formats.SD15())
        default_preview = super().preview(size=size).convert("RGB")
        colour = previewer.decode_latent_to_preview(filtered_noise.cpu())
        default_preview.paste(colour.resize((size[-1], size[-2])), box=(size[-1] * 2, 0))
        return default_preview
